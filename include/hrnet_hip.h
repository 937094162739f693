/*
 * hrnet_hip.h — C ABI of libhrnet_hip.so: the MI355X (gfx950) device path of the HRNet
 * hand-pose hot path.
 *
 * The reference has no FFI on this path: every op below replaces a stock PyTorch op
 * reached from /root/reference/lib/models/pose_hrnet.py, lib/core/loss.py and
 * lib/utils/heatmap_decoding.py (file:line cited per entry point).  The host side
 * (hrnet-hand-pose-estimation_amd/lib/hipnet/) binds these with ctypes; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator) unless it is marked HR_HOST; the library allocates nothing.
 *   - activations are NHWC; `dtype` selects the storage/arithmetic type of activations and
 *     packed weights: HR_F32 (exact f32 MFMA, f32 accumulate) or HR_BF16 (bf16 MFMA, f32
 *     accumulate). Statistics, BN coefficients, partial sums, losses and master weights
 *     are always f32.
 *   - stream-ordered and re-entrant: kernels are enqueued on `stream`, nothing synchronises.
 *   - a function declared `int` returns a status: 0 on success, a negative HR_E_* code otherwise;
 *     hrnet_last_error_string() describes the last failure of the calling thread. Any other return type
 *     (hr_value_t, long long, a pointer) is a value. Nothing throws across the ABI.
 *   - lib/hipnet/_header.py reads this file and the ctypes binding is built from what it finds (prototypes, structs,
 *     enumerators, integer HR_* macros), so the header keeps to the C that reader knows; it refuses the rest.
 */
#ifndef HRNET_HIP_H
#define HRNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HR_ABI_VERSION 2 /* hrnet_abi_version() of a library built from this header */
#define HR_HOST /* on a pointer parameter: host memory the call reads or writes before it returns */

typedef void* hr_stream_t; /* hipStream_t */
typedef int hr_value_t;    /* a count, flag or mode, not a status */

enum { HR_F32 = 0, HR_BF16 = 1 };

enum {
  HR_OK = 0,
  HR_E_BADARG = -1,   /* shape / alignment / dtype the kernels do not support */
  HR_E_LAUNCH = -2,   /* HIP reported a launch error */
  HR_E_BADOP = -3     /* unknown op kind in a program */
};

/* ---- op kinds of a recorded program (hrnet_program_run); the slots of each kind are named below ------ */
enum {
  HR_OP_CONV = 1,          /* conv / dgrad (implicit GEMM, MFMA) */
  HR_OP_WGRAD = 2,         /* weight gradient: partial slabs, or float atomics into the gradient */
  HR_OP_WGRAD_REDUCE = 3,  /* slabs -> OIHW f32 gradient */
  HR_OP_BN_FINALIZE = 4,   /* stat partials -> scale/shift (+ running stats) */
  HR_OP_SUM_TERMS = 5,     /* out = relu(sum_t relu_t(affine_t(up_t(src_t)))) */
  HR_OP_GRAD_TERM = 6,     /* dst (+)= A*pool(g*mask) + B*y + C */
  HR_OP_BN_BWD_REDUCE = 7, /* per-channel sum(dz), sum(dz*y) partials */
  HR_OP_BN_BWD_FINALIZE = 8,
  HR_OP_BILINEAR_CAT = 9,
  HR_OP_BILINEAR_CAT_BWD = 10,
  HR_OP_IM2COL_STEM = 11,
  HR_OP_NHWC_TO_NCHW = 12,
  HR_OP_NCHW_TO_NHWC = 13,
  HR_OP_PACK_WEIGHTS = 14,
  HR_OP_BIAS_GRAD = 15,
  HR_OP_FILL = 16,
  HR_OP_PACK_TABLE = 17,
  HR_OP_EVENT_RECORD = 18,
  HR_OP_STREAM_WAIT = 19,
  HR_OP_WGRAD_REDUCE_TABLE = 20,
  HR_OP_BWD_FUSED = 21,    /* hrnet_conv3x3_bwd_fused */
  HR_OP_BN_FINALIZE_TABLE = 22,
  HR_OP_BWD_PW = 23,       /* hrnet_conv1x1_bwd_fused */
  HR_OP_CONV_SUM = 24,     /* hrnet_conv2d_sum */
  HR_OP_EW_TABLE = 25,     /* several element-wise jobs of one kind as ONE launch */
  HR_OP_HEAD_MIX = 26,     /* hrnet_head_mix */
  HR_OP_UPSAMPLE_T = 27,   /* hrnet_upsample_bilinear_t */
  HR_OP_HEAD_BWD = 28,     /* hrnet_head_bwd */
  HR_OP_POOL_REDUCE = 29   /* pooled BatchNorm-backward reduction of the up-sampled terms of a fuse sum */
};

/* One recorded op: integer / float / pointer slots. What a slot means depends on the kind: the enums below name
 * every slot, HR_<table>_I_* indexing i[], HR_<table>_F_* f[] and HR_<table>_P_* p[] (an argument of the hrnet_*
 * function a table cites keeps that argument's meaning). Kinds that share a layout share a table. A name ending in
 * 0 or 1 is the first member of an indexed family. i[HR_LANE_SLOT] belongs to the runner, not to any kind. */
typedef struct HrOp {
  int32_t kind;
  int32_t i[19];
  float f[4];
  void* p[14];
} HrOp;
#define HR_LANE_SLOT 18

/* slots of HR_OP_CONV: hrnet_conv2d / _bnref / _bwdstats. BS_* (p) make it a backward-statistics launch; such an op
 * may set BS_STORE_MASKED = 1: the stored gradient is dz = v * [mask > 0] (what the fused backward launches expect).
 * IN_DY / IN_DX: displacement of the input window of a 1x1 stride-1 launch (hrnet_conv2d_dilated3x3). ROUTE: the
 * kernel family a recorded backward-statistics launch is bound to (hrnet_conv_route(); 0 = decide at launch).
 * STATS_ATOMIC = 1: STATS is sums[8][2][Cout], added to with float atomics. IN_SUMS / IN_GAMMA / IN_BETA /
 * IN_INV_COUNT / IN_EPS give the input's BatchNorm as batch sums instead of IN_SCALE / IN_SHIFT (hrnet_conv2d_bnref) */
enum { HR_CONV_I_DTYPE = 0, HR_CONV_I_N, HR_CONV_I_H, HR_CONV_I_W, HR_CONV_I_CIN, HR_CONV_I_HO, HR_CONV_I_WO,
       HR_CONV_I_COUT, HR_CONV_I_KS, HR_CONV_I_STRIDE, HR_CONV_I_UPZ, HR_CONV_I_IN_RELU, HR_CONV_I_ACCUMULATE,
       HR_CONV_I_STATS_ATOMIC, HR_CONV_I_BS_STORE_MASKED, HR_CONV_I_IN_DY, HR_CONV_I_IN_DX, HR_CONV_I_ROUTE };
enum { HR_CONV_F_IN_INV_COUNT = 0, HR_CONV_F_IN_EPS };
enum { HR_CONV_P_X = 0, HR_CONV_P_WGT, HR_CONV_P_IN_SCALE, HR_CONV_P_IN_SHIFT, HR_CONV_P_BIAS, HR_CONV_P_Y,
       HR_CONV_P_STATS, HR_CONV_P_BS_Y, HR_CONV_P_BS_MASK, HR_CONV_P_BS_SCALE, HR_CONV_P_BS_SHIFT, HR_CONV_P_IN_SUMS,
       HR_CONV_P_IN_GAMMA, HR_CONV_P_IN_BETA };

/* slots of HR_OP_WGRAD: hrnet_conv2d_wgrad. ATOMIC = 1: SLABS is the OIHW f32 gradient itself
 * ([COUT_REAL][CIN_REAL][ks][ks]) and every workgroup ADDS its tile into it with float atomics - no slabs, no reduce
 * launch, not bit-reproducible; LD (1x1 only): floats between consecutive output-channel rows of that gradient (a
 * column slice of a wider weight), 0 = CIN_REAL */
enum { HR_WGRAD_I_DTYPE = 0, HR_WGRAD_I_N, HR_WGRAD_I_H, HR_WGRAD_I_W, HR_WGRAD_I_CIN, HR_WGRAD_I_HO, HR_WGRAD_I_WO,
       HR_WGRAD_I_COUT, HR_WGRAD_I_KS, HR_WGRAD_I_STRIDE, HR_WGRAD_I_IN_RELU, HR_WGRAD_I_NSPLIT, HR_WGRAD_I_ATOMIC,
       HR_WGRAD_I_COUT_REAL, HR_WGRAD_I_CIN_REAL, HR_WGRAD_I_LD };
enum { HR_WGRAD_P_X = 0, HR_WGRAD_P_DY, HR_WGRAD_P_IN_SCALE, HR_WGRAD_P_IN_SHIFT, HR_WGRAD_P_SLABS };

/* slots of HR_OP_WGRAD_REDUCE: hrnet_wgrad_reduce; LD as HrWredEnt.ld */
enum { HR_WGRAD_REDUCE_I_NSPLIT = 0, HR_WGRAD_REDUCE_I_COUT_PAD, HR_WGRAD_REDUCE_I_CIN_PAD, HR_WGRAD_REDUCE_I_KS,
       HR_WGRAD_REDUCE_I_COUT, HR_WGRAD_REDUCE_I_CIN, HR_WGRAD_REDUCE_I_KFLAT, HR_WGRAD_REDUCE_I_ACCUMULATE,
       HR_WGRAD_REDUCE_I_LD };
enum { HR_WGRAD_REDUCE_P_SLABS = 0, HR_WGRAD_REDUCE_P_GRAD };

/* slots of HR_OP_BN_FINALIZE: hrnet_bn_finalize */
enum { HR_BN_FINALIZE_I_TILES = 0, HR_BN_FINALIZE_I_C, HR_BN_FINALIZE_I_TRAINING };
enum { HR_BN_FINALIZE_F_COUNT = 0, HR_BN_FINALIZE_F_MOMENTUM, HR_BN_FINALIZE_F_EPS };
enum { HR_BN_FINALIZE_P_STATS = 0, HR_BN_FINALIZE_P_GAMMA, HR_BN_FINALIZE_P_BETA, HR_BN_FINALIZE_P_RUNNING_MEAN,
       HR_BN_FINALIZE_P_RUNNING_VAR, HR_BN_FINALIZE_P_NUM_BATCHES_TRACKED, HR_BN_FINALIZE_P_SCALE,
       HR_BN_FINALIZE_P_SHIFT, HR_BN_FINALIZE_P_SAVE_MEAN, HR_BN_FINALIZE_P_SAVE_INVSTD };

/* slots of HR_OP_SUM_TERMS: hrnet_sum_terms / hrnet_sum_terms_bnref; term t < 4 sits at <NAME>0 + t. SUMS_MODE: bit
 * t set = term t's BatchNorm is given as batch sums (SCALE0 + t = sums, SHIFT0 + t = gamma, INV_COUNT0 + t = 1 /
 * count), EPS_BITS = the bits of the f32 eps */
enum { HR_SUM_I_DTYPE = 0, HR_SUM_I_N, HR_SUM_I_H, HR_SUM_I_W, HR_SUM_I_C, HR_SUM_I_NTERMS, HR_SUM_I_RELU_OUT,
       HR_SUM_I_SH0, HR_SUM_I_RELU0 = 11, HR_SUM_I_SUMS_MODE = 15, HR_SUM_I_EPS_BITS };
enum { HR_SUM_F_INV_COUNT0 = 0 };
enum { HR_SUM_P_OUT = 0, HR_SUM_P_SRC0, HR_SUM_P_SCALE0 = 5, HR_SUM_P_SHIFT0 = 9 };

/* slots of HR_OP_GRAD_TERM: hrnet_grad_term and hrnet_grad_term2 (the latter: SH = INNER_RELU = 0, plus DST2 /
 * ACCUMULATE2) */
enum { HR_GRAD_TERM_I_DTYPE = 0, HR_GRAD_TERM_I_N, HR_GRAD_TERM_I_H, HR_GRAD_TERM_I_W, HR_GRAD_TERM_I_C,
       HR_GRAD_TERM_I_SH, HR_GRAD_TERM_I_INNER_RELU, HR_GRAD_TERM_I_ACCUMULATE, HR_GRAD_TERM_I_ACCUMULATE2 };
enum { HR_GRAD_TERM_P_DST = 0, HR_GRAD_TERM_P_G, HR_GRAD_TERM_P_MASK, HR_GRAD_TERM_P_Y, HR_GRAD_TERM_P_SCALE,
       HR_GRAD_TERM_P_SHIFT, HR_GRAD_TERM_P_COEF, HR_GRAD_TERM_P_DST2 };

/* slots of HR_OP_BN_BWD_REDUCE: hrnet_bn_bwd_reduce. DZ (optional): dz itself (pooled, masked, [N,H,W,C] in the
 * compute dtype) stored for the apply pass, which then runs HR_OP_GRAD_TERM with g = that tensor, sh = 0 and no
 * masks (in place). Slots 0..5 of both arrays mean what they mean in HR_OP_GRAD_TERM (one decoder reads both kinds) */
enum { HR_BN_BWD_REDUCE_I_DTYPE = 0, HR_BN_BWD_REDUCE_I_N, HR_BN_BWD_REDUCE_I_H, HR_BN_BWD_REDUCE_I_W,
       HR_BN_BWD_REDUCE_I_C, HR_BN_BWD_REDUCE_I_SH, HR_BN_BWD_REDUCE_I_INNER_RELU };
enum { HR_BN_BWD_REDUCE_P_PARTIALS = 0, HR_BN_BWD_REDUCE_P_G, HR_BN_BWD_REDUCE_P_MASK, HR_BN_BWD_REDUCE_P_Y,
       HR_BN_BWD_REDUCE_P_SCALE, HR_BN_BWD_REDUCE_P_SHIFT, HR_BN_BWD_REDUCE_P_DZ };

/* slots of HR_OP_BN_BWD_FINALIZE: hrnet_bn_bwd_finalize */
enum { HR_BN_BWD_FINALIZE_I_BLOCKS = 0, HR_BN_BWD_FINALIZE_I_C, HR_BN_BWD_FINALIZE_I_ACCUMULATE };
enum { HR_BN_BWD_FINALIZE_F_COUNT = 0 };
enum { HR_BN_BWD_FINALIZE_P_PARTIALS = 0, HR_BN_BWD_FINALIZE_P_GAMMA, HR_BN_BWD_FINALIZE_P_SAVE_MEAN,
       HR_BN_BWD_FINALIZE_P_SAVE_INVSTD, HR_BN_BWD_FINALIZE_P_DGAMMA, HR_BN_BWD_FINALIZE_P_DBETA,
       HR_BN_BWD_FINALIZE_P_COEF };

/* slots of HR_OP_BILINEAR_CAT, HR_OP_BILINEAR_CAT_BWD: hrnet_bilinear_cat / hrnet_bilinear_cat_bwd; branch k < 4 at
 * <NAME>0 + k. ALIGN (a float: != 0 = align_corners); ACCUMULATE: backward only; CAT = the concat (forward) or its
 * gradient, X0 + k = branch k (forward) or its gradient */
enum { HR_CAT_I_DTYPE = 0, HR_CAT_I_NBR, HR_CAT_I_N, HR_CAT_I_H, HR_CAT_I_W, HR_CAT_I_HS0, HR_CAT_I_WS0 = 9,
       HR_CAT_I_CS0 = 13, HR_CAT_I_ACCUMULATE = 17 };
enum { HR_CAT_F_ALIGN = 0 };
enum { HR_CAT_P_CAT = 0, HR_CAT_P_X0 };

/* slots of HR_OP_IM2COL_STEM: hrnet_im2col_stem */
enum { HR_IM2COL_I_DTYPE = 0, HR_IM2COL_I_N, HR_IM2COL_I_C, HR_IM2COL_I_H, HR_IM2COL_I_W, HR_IM2COL_I_HO,
       HR_IM2COL_I_WO, HR_IM2COL_I_KPAD };
enum { HR_IM2COL_P_IMG = 0, HR_IM2COL_P_COLS };

/* slots of HR_OP_NHWC_TO_NCHW, HR_OP_NCHW_TO_NHWC: hrnet_nhwc_to_nchw / hrnet_nchw_to_nhwc */
enum { HR_LAYOUT_I_DTYPE = 0, HR_LAYOUT_I_N, HR_LAYOUT_I_H, HR_LAYOUT_I_W, HR_LAYOUT_I_CP, HR_LAYOUT_I_C };
enum { HR_LAYOUT_P_SRC = 0, HR_LAYOUT_P_DST };

/* slots of HR_OP_PACK_WEIGHTS: hrnet_pack_weights */
enum { HR_PACK_I_DTYPE = 0, HR_PACK_I_COUT, HR_PACK_I_CIN, HR_PACK_I_KS, HR_PACK_I_COUT_PAD, HR_PACK_I_CIN_PAD,
       HR_PACK_I_MODE };
enum { HR_PACK_P_SRC = 0, HR_PACK_P_PACKED };

/* slots of HR_OP_BIAS_GRAD: hrnet_bias_grad */
enum { HR_BIAS_GRAD_I_DTYPE = 0, HR_BIAS_GRAD_I_PIXELS, HR_BIAS_GRAD_I_CP, HR_BIAS_GRAD_I_C,
       HR_BIAS_GRAD_I_ACCUMULATE };
enum { HR_BIAS_GRAD_P_DY = 0, HR_BIAS_GRAD_P_DBIAS, HR_BIAS_GRAD_P_SCRATCH };

/* slots of HR_OP_FILL: hrnet_fill_zero: the byte count as two 32-bit halves */
enum { HR_FILL_I_BYTES_LO = 0, HR_FILL_I_BYTES_HI };
enum { HR_FILL_P_DST = 0 };

/* slots of HR_OP_PACK_TABLE: hrnet_pack_weights_table (TABLE: device HrPackEnt[N]) */
enum { HR_PACK_TABLE_I_DTYPE = 0, HR_PACK_TABLE_I_N, HR_PACK_TABLE_I_BLOCKS };
enum { HR_PACK_TABLE_P_TABLE = 0 };

/* slots of HR_OP_EVENT_RECORD, HR_OP_STREAM_WAIT: EVENT (from hrnet_event_create) is recorded on the op's lane / the
 * op's lane waits for it */
enum { HR_EVENT_P_EVENT = 0 };

/* slots of HR_OP_WGRAD_REDUCE_TABLE, HR_OP_BN_FINALIZE_TABLE: hrnet_wgrad_reduce_table (TABLE: device HrWredEnt[N])
 * / hrnet_bn_finalize_table (device HrBnEnt[N]); BLOCKS = total blocks */
enum { HR_TABLE_I_N = 0, HR_TABLE_I_BLOCKS };
enum { HR_TABLE_P_TABLE = 0 };

/* slots of HR_OP_BWD_FUSED, HR_OP_BWD_PW: hrnet_conv3x3_bwd_fused / hrnet_conv1x1_bwd_fused (HR_OP_BWD_PW: pixels =
 * N * H * W). BNREF: HOST pointer to a HrBnBwdRef kept alive by the caller, or NULL. ATOMIC = 1: SLABS is the OIHW
 * gradient the weight-gradient tiles are ADDED to (float atomics), COUT_REAL / CIN_REAL its extents (HR_OP_BWD_PW:
 * they must equal the tensors') */
enum { HR_BWD_FUSED_I_DTYPE = 0, HR_BWD_FUSED_I_N, HR_BWD_FUSED_I_H, HR_BWD_FUSED_I_W, HR_BWD_FUSED_I_CIN,
       HR_BWD_FUSED_I_COUT, HR_BWD_FUSED_I_IN_RELU, HR_BWD_FUSED_I_MASK_OUT, HR_BWD_FUSED_I_ATOMIC,
       HR_BWD_FUSED_I_COUT_REAL, HR_BWD_FUSED_I_CIN_REAL };
enum { HR_BWD_FUSED_P_DZ = 0, HR_BWD_FUSED_P_Y, HR_BWD_FUSED_P_COEF, HR_BWD_FUSED_P_X, HR_BWD_FUSED_P_IN_SCALE,
       HR_BWD_FUSED_P_IN_SHIFT, HR_BWD_FUSED_P_WT, HR_BWD_FUSED_P_DX, HR_BWD_FUSED_P_ADDEND, HR_BWD_FUSED_P_ROWS,
       HR_BWD_FUSED_P_BS_Y, HR_BWD_FUSED_P_SLABS, HR_BWD_FUSED_P_BNREF };

/* slots of HR_OP_CONV_SUM: hrnet_conv2d_sum */
enum { HR_CONV_SUM_I_DTYPE = 0, HR_CONV_SUM_I_N, HR_CONV_SUM_I_H, HR_CONV_SUM_I_W, HR_CONV_SUM_I_CIN,
       HR_CONV_SUM_I_COUT, HR_CONV_SUM_I_KS, HR_CONV_SUM_I_STATS_ATOMIC };
enum { HR_CONV_SUM_F_IN_INV_COUNT = 0, HR_CONV_SUM_F_IN_EPS };
enum { HR_CONV_SUM_P_X = 0, HR_CONV_SUM_P_WGT, HR_CONV_SUM_P_IN_SCALE, HR_CONV_SUM_P_IN_SHIFT, HR_CONV_SUM_P_IN_SUMS,
       HR_CONV_SUM_P_IN_GAMMA, HR_CONV_SUM_P_IN_BETA, HR_CONV_SUM_P_Y, HR_CONV_SUM_P_STATS, HR_CONV_SUM_P_X2,
       HR_CONV_SUM_P_SIDE };

/* slots of HR_OP_EW_TABLE: several HR_OP_GRAD_TERM / HR_OP_BN_BWD_REDUCE / HR_OP_BN_BWD_FINALIZE / HR_OP_POOL_REDUCE
 * / HR_OP_SUM_TERMS jobs as ONE launch. TABLE: device array of JOBS HrOp records of kind KIND (slots as for the
 * single op, plus HR_EWJOB_* below); BLOCKS = total blocks; SUMS (HR_OP_SUM_TERMS) = 1 if some job's BatchNorm is
 * given as batch sums */
enum { HR_EW_TABLE_I_JOBS = 0, HR_EW_TABLE_I_BLOCKS, HR_EW_TABLE_I_KIND, HR_EW_TABLE_I_DTYPE, HR_EW_TABLE_I_SUMS };
enum { HR_EW_TABLE_P_TABLE = 0 };

/* slots of HR_OP_HEAD_MIX: hrnet_head_mix; up-sampled term k < 3: UP_H1 + 2 * k, UP_W1 + 2 * k, T1 + k */
enum { HR_HEAD_MIX_I_DTYPE = 0, HR_HEAD_MIX_I_N, HR_HEAD_MIX_I_H, HR_HEAD_MIX_I_W, HR_HEAD_MIX_I_C0,
       HR_HEAD_MIX_I_COUT, HR_HEAD_MIX_I_NUP, HR_HEAD_MIX_I_ALIGN, HR_HEAD_MIX_I_UP_H1, HR_HEAD_MIX_I_UP_W1,
       HR_HEAD_MIX_I_ROWS_MODE = 14 };
enum { HR_HEAD_MIX_P_X0 = 0, HR_HEAD_MIX_P_W0, HR_HEAD_MIX_P_BIAS, HR_HEAD_MIX_P_Y, HR_HEAD_MIX_P_STATS,
       HR_HEAD_MIX_P_T1 };

/* slots of HR_OP_UPSAMPLE_T: hrnet_upsample_bilinear_t; output k < 3: OUT_H1 + 2 * k, OUT_W1 + 2 * k, OUT1 + k */
enum { HR_UPSAMPLE_T_I_DTYPE = 0, HR_UPSAMPLE_T_I_N, HR_UPSAMPLE_T_I_H, HR_UPSAMPLE_T_I_W, HR_UPSAMPLE_T_I_C,
       HR_UPSAMPLE_T_I_NOUT, HR_UPSAMPLE_T_I_ALIGN, HR_UPSAMPLE_T_I_OUT_H1, HR_UPSAMPLE_T_I_OUT_W1,
       HR_UPSAMPLE_T_I_STREAMED = 13 };
enum { HR_UPSAMPLE_T_P_G = 0, HR_UPSAMPLE_T_P_OUT1 };

/* slots of HR_OP_HEAD_BWD: hrnet_head_bwd */
enum { HR_HEAD_BWD_I_DTYPE = 0, HR_HEAD_BWD_I_N, HR_HEAD_BWD_I_H, HR_HEAD_BWD_I_W, HR_HEAD_BWD_I_K,
       HR_HEAD_BWD_I_COUT, HR_HEAD_BWD_I_MODE, HR_HEAD_BWD_I_INNER_RELU };
enum { HR_HEAD_BWD_P_DY = 0, HR_HEAD_BWD_P_WT, HR_HEAD_BWD_P_Y, HR_HEAD_BWD_P_OUT, HR_HEAD_BWD_P_BN_SCALE,
       HR_HEAD_BWD_P_BN_SHIFT, HR_HEAD_BWD_P_COEF };

/* slots of HR_OP_POOL_REDUCE: the BatchNorm-backward reduction of up to three nearest-up-sampled terms of one fuse
 * sum (pose_hrnet.py:257-264) in ONE walk over the sum's gradient G: level l < NLEV pools 2^(l+1) x 2^(l+1) blocks
 * and sits at Y0 / DZ0 / PARTIALS0 + 3 * l; dz_l is stored for the apply pass (HR_OP_GRAD_TERM with g = dz_l, sh =
 * 0); partials_l[hrnet_reduce_blocks(N, H / 2, W / 2, C)][2][C] */
enum { HR_POOL_I_DTYPE = 0, HR_POOL_I_N, HR_POOL_I_H, HR_POOL_I_W, HR_POOL_I_C, HR_POOL_I_NLEV };
enum { HR_POOL_P_G = 0, HR_POOL_P_MASK, HR_POOL_P_Y0, HR_POOL_P_DZ0, HR_POOL_P_PARTIALS0 };

/* A job of a HR_OP_EW_TABLE launch is an HrOp of the jobs' kind in the device table with its block range laid over
 * it: blocks [BLOCK0, BLOCK0 + BLOCKS) of the launch are the job's (BLOCKS = hrnet_ew_table_blocks()). No table of a
 * kind that can be a job names these two slots - except HR_SUM_I_EPS_BITS, which a sum job therefore carries in
 * SUM_EPS_BITS instead (a job has no lane). */
enum { HR_EWJOB_I_BLOCK0 = 16, HR_EWJOB_I_BLOCKS = 17, HR_EWJOB_I_SUM_EPS_BITS = 18 };

const char* hrnet_last_error_string(void);
hr_value_t hrnet_abi_version(void);

/* Run `n` recorded ops in order on `stream` (one host call per forward / backward pass). */
int hrnet_program_run(HR_HOST const HrOp* ops, int n, hr_stream_t stream);
/* blocks of one job of a HR_OP_EW_TABLE launch (kind = the single op's kind; finalize: N = H = W = 1) */
hr_value_t hrnet_ew_table_blocks(int kind, int dtype, int N, int H, int W, int C);
/* The same over several streams: op.i[HR_LANE_SLOT] selects streams[lane]; HR_OP_EVENT_RECORD /
 * HR_OP_STREAM_WAIT ops express the dependencies between lanes (independent branches of a
 * HighResolutionModule, weight-gradient work off the critical path). Events come from
 * hrnet_event_create (host-side handles; no device memory). */
int hrnet_program_run_streams(HR_HOST const HrOp* ops, int n, HR_HOST const hr_stream_t* streams, int nstreams);
/* Measurement form of the above: a timing event behind every op on its lane; end_ms[k] = completion of op k in
 * ms since the call began on op 0's lane. Synchronises every stream before returning (not for the training loop). */
int hrnet_program_run_streams_timed(HR_HOST const HrOp* ops, int n, HR_HOST const hr_stream_t* streams, int nstreams,
                                    HR_HOST float* end_ms);
void* hrnet_event_create(void);
int hrnet_event_destroy(void* event);

/*
 * Convolution as implicit GEMM on MFMA. Replaces nn.Conv2d forward (pose_hrnet.py:22-25,
 * :65-71, :200-204, :218-222, :283-287, :334-347) and, with packed transposed weights, its
 * input gradient.
 *   x        [N,H,W,Cin]   (Cin % 8 == 0; HR_F32: % 4)
 *   w        packed [Cout][ks*ks][Cin] in `dtype` (hrnet_pack_weights)
 *   in_scale/in_shift  optional per-Cin affine applied to x on load (the producer's
 *            BatchNorm, pose_hrnet.py:45,49 ...), then ReLU if in_relu; zero padding is
 *            applied AFTER the transform, as the reference pads the activated tensor.
 *   bias     optional [Cout] f32
 *   y        [N,Ho,Wo,Cout] (Cout % 16 == 0), overwritten or accumulated into
 *   stats    optional [tiles][2][Cout] f32 per-tile sum / sum of squares of y (BatchNorm
 *            batch statistics, finished by hrnet_bn_finalize); tiles = hrnet_conv_tiles()
 *   ks 1|3, pad = ks/2, stride 1|2.  upz=1: x is read as if zero-stuffed x2 (input gradient
 *   of a stride-2 conv: logical input [N,Ho,Wo,Cin], stride forced to 1).
 */
int hrnet_conv2d(int dtype, const void* x, const void* w, const float* in_scale,
                 const float* in_shift, const float* bias, void* y, float* stats, int N, int H,
                 int W, int Cin, int Ho, int Wo, int Cout, int ks, int stride, int upz,
                 int in_relu, int accumulate, hr_stream_t stream);

/* out[i] = sum_{j<k} coefs[j] * srcs[j][i], f32, k <= 8 (host arrays of k device pointers / k coefficients): the
 * frame differences and the weighted temporal aggregation of pose_hrnet_PoseAggr
 * (lib/models/pose_hrnet_PoseAggr.py:612-640) */
int hrnet_lincomb_f32(float* out, long long n, int k, HR_HOST const float* const* srcs, HR_HOST const float* coefs,
                      hr_stream_t stream);

/*
 * 3x3 convolution with dilation d and padding d (the offset-generating convs of pose_hrnet_PoseAggr,
 * lib/models/pose_hrnet_PoseAggr.py:497-506: dilations 3, 6, 12, 18, 24; a halo of d pixels does not fit the tiled
 * conv body): nine 1x1 launches over input windows displaced by ((r-1)d, (s-1)d), accumulating into y.
 *   w_taps: nine packed 1x1 weight matrices [Cout][Cin] (hrnet_pack_weights mode 0 of w[:, :, r, s]), tap t = 3r+s
 *   at w_taps + t * tap_stride_bytes. No bias / BatchNorm prologue; y is rounded to `dtype` between taps.
 */
int hrnet_conv2d_dilated3x3(int dtype, const void* x, const void* w_taps, long long tap_stride_bytes, void* y,
                            int N, int H, int W, int Cin, int Cout, int dilation, hr_stream_t stream);

/*
 * Input-gradient convolution that also gathers the statistics of the BatchNorm backward pass of
 * its output (autograd of pose_hrnet.py:43-57 - the reduction half of native_batch_norm_backward):
 * y (overwritten or accumulated) is the gradient v of an activation; stats rows receive
 * (sum dz, sum dz*yraw) per channel with dz = v * [m > 0], m = bs_mask (or bs_y when bs_mask is
 * NULL) optionally mapped through bs_scale/bs_shift; no mask at all when bs_mask and bs_scale are
 * both NULL. bs_y / bs_mask are laid out like y. Rows are finished by hrnet_bn_bwd_finalize with
 * blocks = hrnet_conv_tiles_bwdstats(N,Ho,Wo,Cout,ks,stride).
 */
int hrnet_conv2d_bwdstats(int dtype, const void* x, const void* w, void* y, float* stats,
                          const void* bs_y, const void* bs_mask, const float* bs_scale,
                          const float* bs_shift, int N, int H, int W, int Cin, int Ho, int Wo,
                          int Cout, int ks, int stride, int upz, int accumulate, hr_stream_t stream);
/*
 * The 3x3 stride-1 branch convolutions (BasicBlock.conv1 / conv2, pose_hrnet.py:41-57) run as an LDS-ring
 * pipeline (csrc/conv_ring.hip) behind hrnet_conv2d / hrnet_conv2d_bnref when the shape is served (bf16, Cin a
 * multiple of 32, no bias / accumulate / zero-stuffing, output statistics by atomics or none). This switch turns
 * that routing on (1, the default; environment HRNET_CONV_RING) or off (0: the tile-walking body of conv_body.h)
 * for A/B measurements and parity tests; 2: on, and the >= 96-channel 16x16-tile instantiation also takes maps larger
 * than 16x16 (it serves them correctly but loses inside the training step, so 1 keeps it to 16x16 maps). Returns the
 * previous setting (-1: never decided).
 */
hr_value_t hrnet_conv_ring_enable(int on);
hr_value_t hrnet_conv_ring_supported(int dtype, int N, int H, int W, int Cin, int Cout);
/* statistics rows hrnet_conv2d_bwdstats leaves for a launch of this shape (hrnet_conv_tiles_bwdstats() for the
 * tile-walking body; the pixel walks of the LDS-ring grid where that serves the launch) */
hr_value_t hrnet_conv_rows_bwdstats(int dtype, int N, int Ho, int Wo, int Cin, int Cout, int ks, int stride);
/* kernel family a RECORDED backward-statistics launch of this shape is bound to (HR_CONV_I_ROUTE): 2 = LDS ring,
 * 1 = tile-walking body; the rows buffer above is sized for that family, so the op keeps the decision and a later
 * hrnet_conv_ring_enable() cannot change how many rows the launch writes (it fails instead). 0 = decide at launch. */
hr_value_t hrnet_conv_route(int dtype, int N, int Ho, int Wo, int Cin, int Cout, int ks, int stride);
/* hrnet_conv2d_sum on the LDS-ring pipeline for the narrow branch layers (bf16, 3x3, 32 / 64 input channels): off by
 * default (measured slower inside the training step), on = 1; returns the previous setting */
hr_value_t hrnet_conv_ring_sum_enable(int on);

/* name of the kernel instantiation chosen for a shape, as rocprofv3 demangles it (returns length) */
hr_value_t hrnet_conv_kernel_name(int dtype, int N, int Ho, int Wo, int Cin, int Cout, int ks, int stride, int upz,
                                  int mode, HR_HOST char* buf, int buflen);
/* the specialised kernel family a conv launch uses: 0 conv_kernel (everything by run-time flag), 1
 * conv_bs_kernel (backward statistics), 2 conv_fwd_kernel (forward conv feeding a BatchNorm), 3
 * conv_dg_kernel (plain input gradient), 4 conv_fwdb_kernel (forward conv with bias) */
hr_value_t hrnet_conv_mode(int bwdstats, int has_bias, int upz, int accumulate, int has_stats, int has_affine,
                           int in_relu);
hr_value_t hrnet_wgrad_kernel_name(int dtype, int Ho, int Wo, int Cout, int Cin, int ks, int stride,
                                   HR_HOST char* buf, int buflen);
/* number of per-tile stat rows hrnet_conv2d writes for this shape */
hr_value_t hrnet_conv_tiles(int N, int Ho, int Wo, int Cout, int ks, int stride);
/* the tile walk of a conv launch: out5 = {tile h, tile w, output-channel block, pixel tiles per workgroup,
 * pixel walks (= statistics rows)}; returns the number of pixel tiles. s2d = the four-parity input gradient
 * of a 3x3 stride-2 conv (upz with hrnet_conv2d_bwdstats or a plain input-gradient launch). */
hr_value_t hrnet_conv_tile_walk(int N, int Ho, int Wo, int Cout, int ks, int stride, int bwdstats, int s2d,
                                HR_HOST int* out5);
/* rows of a hrnet_conv2d_bwdstats launch (its tile choice differs for wide 1x1 outputs) */
hr_value_t hrnet_conv_tiles_bwdstats(int N, int Ho, int Wo, int Cout, int ks, int stride);

/*
 * Weight gradient: slabs[s][Cout][ks*ks][Cin] f32 partial sums over disjoint pixel ranges
 * (deterministic, no atomics); x is transformed on load exactly as in hrnet_conv2d.
 *   dy [N,Ho,Wo,Cout], x [N,H,W,Cin]; nsplit slabs = hrnet_wgrad_splits().
 */
int hrnet_conv2d_wgrad(int dtype, const void* x, const void* dy, const float* in_scale,
                       const float* in_shift, float* slabs, int N, int H, int W, int Cin, int Ho,
                       int Wo, int Cout, int ks, int stride, int in_relu, int nsplit,
                       hr_stream_t stream);
hr_value_t hrnet_wgrad_splits(int dtype, int N, int Ho, int Wo, int Cout, int Cin, int ks, int stride);
/* pixel tiles the launch walks in all (a split takes tiles / nsplit of them, grid-strided) */
hr_value_t hrnet_wgrad_tiles(int dtype, int N, int Ho, int Wo, int Cout, int Cin, int ks, int stride);
/* workgroups per split (a launch runs splits x this many) */
hr_value_t hrnet_wgrad_blocks_per_split(int dtype, int Ho, int Wo, int Cout, int Cin, int ks, int stride);
/* slabs -> grad_oihw[Cout_real][Cin_real][ks][ks] f32 (+= if accumulate). Cout/Cin are the
 * padded slab extents; stem: kflat=1 means slab K index is the flattened (tap,ci) of the
 * im2col'ed stem (Cin_real*ks*ks real entries). */
int hrnet_wgrad_reduce(const float* slabs, float* grad_oihw, int nsplit, int Cout, int Cin,
                       int ks, int Cout_real, int Cin_real, int kflat, int accumulate,
                       hr_stream_t stream);

/*
 * Fused backward of a 3x3 stride-1 convolution y = conv(a), a = relu?(in_scale*x + in_shift), whose output
 * feeds a BatchNorm (autograd of the BasicBlock body, pose_hrnet.py:41-57): ONE launch applies the BatchNorm
 * backward to the upstream gradient while staging it (g = A*dz + B*y + C with coef = [3][Cout] of
 * hrnet_bn_bwd_finalize; coef NULL: g = dz), forms the weight-gradient slabs (layout and reduction as
 * hrnet_conv2d_wgrad; nsplit = hrnet_bwd_fused_splits()), the input gradient (+ `addend`, the residual
 * stream), masks it with [a > 0] when mask_out (so what is stored is the dz of the NEXT BatchNorm backward)
 * and, when `rows` is given, leaves (sum dx, sum dx*bs_y) per channel in rows[nsplit][2][Cin] for
 * hrnet_bn_bwd_finalize (bs_y NULL: the second sum is 0).
 *   dz, y [N,H,W,Cout]; x, dx, addend, bs_y [N,H,W,Cin]; wT = hrnet_pack_weights(mode 1) of the conv.
 * dz must already carry the ReLU mask of the BatchNorm output it belongs to (an in-place hrnet_grad_term with
 * coef NULL does that where the producer did not). Served shapes: hrnet_bwd_fused_supported().
 */
int hrnet_conv3x3_bwd_fused(int dtype, const void* dz, const void* y, const float* coef, const void* x,
                            const float* in_scale, const float* in_shift, int in_relu, const void* wT, void* dx,
                            const void* addend, int mask_out, float* rows, const void* bs_y, float* slabs, int N,
                            int H, int W, int Cin, int Cout, hr_stream_t stream);
hr_value_t hrnet_bwd_fused_supported(int dtype, int Cin, int Cout);
/*
 * The fused launches can finish the BatchNorm backward of their own output themselves: instead of `coef` (written by
 * a hrnet_bn_bwd_finalize launch in between) they take the partial rows [nrows][2][Cout] the previous launch left
 * - every workgroup sums them in a fixed order (f64) and builds A,B,C itself; the first workgroup also adds
 * dgamma / dbeta. Same arithmetic as hrnet_bn_bwd_finalize, deterministic, one launch and one dependency less per
 * BatchNorm. `ref` is a HOST struct copied into the launch; NULL = use `coef`. It is not marked HR_HOST: a recorded
 * op carries it as an address (HR_BWD_FUSED_P_BNREF), and callers of the direct form pass the address too. Keep
 * nrows * Cout <= 16384 (3x3) / 8192 (1x1): every workgroup reads all rows.
 */
typedef struct HrBnBwdRef {
  const float* rows;    /* [nrows][2][Cout]: (sum dz, sum dz*y) partials */
  const float* gamma;
  const float* save_mean;
  const float* save_invstd;
  float* dgamma;        /* += (accumulate) or = */
  float* dbeta;
  float count;          /* elements per channel */
  int32_t nrows, accumulate, reserved;
} HrBnBwdRef;
int hrnet_conv3x3_bwd_fused_bnref(int dtype, const void* dz, const void* y, const float* coef, const HrBnBwdRef* ref,
                                  const void* x, const float* in_scale, const float* in_shift, int in_relu,
                                  const void* wT, void* dx, const void* addend, int mask_out, float* rows,
                                  const void* bs_y, float* slabs, int N, int H, int W, int Cin, int Cout,
                                  hr_stream_t stream);
hr_value_t hrnet_bwd_fused_splits(int dtype, int N, int H, int W, int Cin, int Cout);
hr_value_t hrnet_bwd_fused_kernel_name(int dtype, int Cin, int Cout, HR_HOST char* buf, int buflen);

/*
 * The same fused backward for a 1x1 (pointwise) convolution: the conv1 / conv3 / downsample layers of a
 * Bottleneck (autograd of pose_hrnet.py:60-105). Pixels are a flat index: dz, y [pixels,Cout]; x, dx, addend,
 * bs_y [pixels,Cin]; wT = hrnet_pack_weights(mode 1) of the 1x1 kernel ([Cin][Cout]); slabs
 * [hrnet_bwd_pw_splits()][Cout][Cin] f32 (sum with hrnet_wgrad_reduce, ks = 1). bf16 only; served shapes
 * (Cin,Cout) = (64,256), (256,64), (64,64): hrnet_bwd_pw_supported(). `rows` (the next BatchNorm's backward sums,
 * [splits][2][Cin]) where hrnet_bwd_pw_rows_supported() (every served shape).
 */
int hrnet_conv1x1_bwd_fused(int dtype, const void* dz, const void* y, const float* coef, const void* x,
                            const float* in_scale, const float* in_shift, int in_relu, const void* wT, void* dx,
                            const void* addend, int mask_out, float* rows, const void* bs_y, float* slabs,
                            long long pixels, int Cin, int Cout, hr_stream_t stream);
int hrnet_conv1x1_bwd_fused_bnref(int dtype, const void* dz, const void* y, const float* coef, const HrBnBwdRef* ref,
                                  const void* x, const float* in_scale, const float* in_shift, int in_relu,
                                  const void* wT, void* dx, const void* addend, int mask_out, float* rows,
                                  const void* bs_y, float* slabs, long long pixels, int Cin, int Cout,
                                  hr_stream_t stream);
hr_value_t hrnet_bwd_pw_supported(int dtype, int Cin, int Cout);
hr_value_t hrnet_bwd_pw_rows_supported(int dtype, int Cin, int Cout);
hr_value_t hrnet_bwd_pw_splits(int dtype, long long pixels, int Cin, int Cout);
hr_value_t hrnet_bwd_pw_kernel_name(int dtype, int Cin, int Cout, HR_HOST char* buf, int buflen);

/*
 * Pack f32 OIHW master weights into the kernels' layout.
 *   mode 0: forward  [Cout_pad][ks*ks][Cin_pad]
 *   mode 1: dgrad    [Cin_pad][ks*ks flipped][Cout_pad]  (transposed conv)
 *   mode 2: stem     [Cout_pad][Cin_pad] with k = (r*ks+s)*Cin_real + ci  (im2col order)
 */
int hrnet_pack_weights(int dtype, const float* w_oihw, void* packed, int Cout, int Cin, int ks,
                       int Cout_pad, int Cin_pad, int mode, hr_stream_t stream);
/* The same for every convolution of a network in ONE launch: `table` is a DEVICE array of n
 * entries; entry e covers blocks [block0, block0 + hrnet_pack_blocks(Cout_pad, Cin_pad, ks, mode));
 * total_blocks = their sum. A block stages a master row (mode 0: Cin*ks*ks floats) or 4/2/1 input channels of
 * every output channel (mode 1: Cout_pad * (n*ks*ks + 1) floats) in 19 KB of LDS: Cin*ks*ks and
 * Cout_pad*(ks*ks+1) must not exceed 4864. */
typedef struct HrPackEnt {
  const void* w;   /* f32 OIHW master weights */
  void* out;       /* packed weights */
  int32_t Cout, Cin, ks, Cout_pad, Cin_pad, mode, block0;
  int32_t ld;      /* mode 0: floats between consecutive output-channel rows of w (a column slice of a wider 1x1
                      weight); 0 = dense OIHW */
} HrPackEnt;
int hrnet_pack_weights_table(int dtype, const HrPackEnt* table, int n, int total_blocks,
                             hr_stream_t stream);
hr_value_t hrnet_pack_blocks(int Cout_pad, int Cin_pad, int ks, int mode);

/* hrnet_wgrad_reduce for many convolutions in ONE launch (each layer keeps its own slab region):
 * `table` is a DEVICE array of n entries; entry e covers blocks [block0, block0 +
 * ceil(Cout*Cin*ks*ks / 64)); total_blocks = their sum. Same element order and summation tree as
 * hrnet_wgrad_reduce, so the result is bit-identical to the per-layer call. */
typedef struct HrWredEnt {
  const float* slabs; /* [nsplit][Cout_pad][taps][Cin_pad] (kflat: [nsplit][Cout_pad][Cin_pad]) */
  float* grad;        /* OIHW f32 [Cout][Cin][ks][ks] */
  int32_t nsplit, Cout_pad, Cin_pad, ks, Cout, Cin, kflat, accumulate, block0;
  int32_t ld;         /* floats between consecutive output-channel rows of grad (column slice); 0 = dense */
} HrWredEnt;
int hrnet_wgrad_reduce_table(const HrWredEnt* table, int n, int total_blocks, hr_stream_t stream);

/*
 * BatchNorm2d statistics -> per-channel affine (nn.BatchNorm2d in pose_hrnet.py:34,37,66-73,
 * :205,:223,:285-288,:340; momentum 0.1, eps 1e-5).
 *   training=1: mean/var from `stats` ([tiles][2][C], `count` elements per channel);
 *               running_mean/var updated in place (unbiased var), num_batches_tracked += 1
 *   training=0: scale/shift from the running statistics.
 *   scale = gamma*invstd, shift = beta - mean*scale; save_mean/save_invstd kept for backward.
 */
int hrnet_bn_finalize(const float* stats, int tiles, int C, float count, const float* gamma,
                      const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float momentum, float eps, int training,
                      float* scale, float* shift, float* save_mean, float* save_invstd,
                      hr_stream_t stream);

/*
 * Consumer-side BatchNorm: instead of a finalize launch after every conv, a producer accumulates its batch sums
 * into sums[8][2][C] with float atomics (hrnet_conv2d_bnref: out_sums, zeroed by the caller before the pass) and
 * every forward consumer turns sums + gamma/beta into scale/shift itself (one table per workgroup). ONE
 * hrnet_bn_finalize_table launch at the end of the pass fills, for every BatchNorm of the table, the arrays the
 * backward pass reads (scale, shift, save_mean, save_invstd) and updates the running statistics - with the same
 * arithmetic, so both passes see identical coefficients. Atomic accumulation makes the last bits of the batch
 * statistics run-to-run dependent (like cuDNN's); hrnet_conv2d + hrnet_bn_finalize remain the deterministic form.
 *   hrnet_conv2d_bnref: hrnet_conv2d with the input affine given as (in_sums, in_gamma, in_beta, 1/count, eps)
 *   (NULL in_sums: no input BatchNorm) and the output statistics added into out_sums (NULL: none).
 */
int hrnet_conv2d_bnref(int dtype, const void* x, const void* w, const float* in_sums, const float* in_gamma,
                       const float* in_beta, float in_inv_count, float in_eps, const float* bias, void* y,
                       float* out_sums, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int ks, int stride,
                       int in_relu, hr_stream_t stream);
/*
 * Forward conv (3x3 or 1x1, stride 1) whose input is the residual sum that closes the previous block, formed in
 * the conv's own prologue: a = relu(bn(x) + x2) with bn given as scale/shift arrays OR as batch sums + gamma/beta
 * (as hrnet_conv2d_bnref), y = conv(a) (+ statistics of y: rows, or sums[8][2][Cout] when stats_atomic), and `side`
 * = a, written once per pixel - the tensor the next residual add and the backward pass read. Replaces
 * hrnet_sum_terms(relu(bn(x) + x2)) followed by hrnet_conv2d: one launch and one tensor read less
 * (pose_hrnet.py:54-55 + :44 of the next BasicBlock; :95-96 + :79 for Bottlenecks).
 *   x, x2, side [N,H,W,Cin]; y [N,H,W,Cout]; stats may be NULL (eval mode).
 */
int hrnet_conv2d_sum(int dtype, const void* x, const void* x2, const void* w, const float* in_scale,
                     const float* in_shift, const float* in_sums, const float* in_gamma, const float* in_beta,
                     float in_inv_count, float in_eps, void* side, void* y, float* stats, int stats_atomic, int N,
                     int H, int W, int Cin, int Cout, int ks, hr_stream_t stream);

typedef struct HrBnEnt {
  const float* sums;   /* [8][2][C]; NULL: eval mode - scale/shift from running_mean/var, nothing else written */
  const float* gamma;
  const float* beta;
  float* running_mean; /* may be NULL */
  float* running_var;
  int64_t* num_batches_tracked; /* may be NULL */
  float* scale;
  float* shift;
  float* mean;
  float* invstd;
  float count, momentum, eps;
  int32_t C, block0, reserved;
} HrBnEnt;
/* `table`: DEVICE array of n entries; entry e covers blocks [block0, block0 + ceil(C/256)); total_blocks = sum */
int hrnet_bn_finalize_table(const HrBnEnt* table, int n, int total_blocks, hr_stream_t stream);
/* hrnet_sum_terms with BatchNorm terms given as batch sums: bit t of sums_mode set -> scale[t] = sums[8][2][C],
 * shift[t] = gamma (beta = gamma + C), inv_counts[t] = 1 / (elements per channel of term t) */
int hrnet_sum_terms_bnref(int dtype, void* out, int N, int Ho, int Wo, int C, int nterms,
                          HR_HOST const void* const* src, HR_HOST const float* const* scale,
                          HR_HOST const float* const* shift, HR_HOST const int* shifts, HR_HOST const int* relus,
                          int relu_out, int sums_mode, HR_HOST const float* inv_counts, float eps, hr_stream_t stream);

/*
 * out[N,Ho,Wo,C] = relu_out( sum_{t<nterms} relu_t( src_t[nearest-up by 2^sh_t] * scale_t + shift_t ) )
 * Residual adds (pose_hrnet.py:54-55, :95-96) and fuse-layer sums with nearest upsampling
 * (pose_hrnet.py:257-264, :206). scale_t may be NULL (identity term).
 */
int hrnet_sum_terms(int dtype, void* out, int N, int Ho, int Wo, int C, int nterms,
                    HR_HOST const void* const* src, HR_HOST const float* const* scale,
                    HR_HOST const float* const* shift, HR_HOST const int* shifts, HR_HOST const int* relus,
                    int relu_out, hr_stream_t stream);

/*
 * Backward of one term of hrnet_sum_terms / of a BN(+ReLU) that feeds a conv:
 *   dz[q,c]  = sum_{p in 2^sh x 2^sh block of q} g[p,c] * [mask_out[p,c] > 0] * [scale*y+shift > 0 if inner_relu]
 *   dst[q,c] (+)= A[c]*dz + B[c]*y[q,c] + C[c]          (coef = [3][C] from hrnet_bn_bwd_finalize;
 *                                                        coef NULL: dst (+)= dz)
 * g, mask_out: [N,H<<sh,W<<sh,C]; y, dst: [N,H,W,C].
 */
int hrnet_grad_term(int dtype, void* dst, const void* g, const void* mask_out, const void* y,
                    const float* scale, const float* shift, const float* coef, int N, int H, int W,
                    int C, int sh, int inner_relu, int accumulate, hr_stream_t stream);
/* same with sh = 0 and no inner ReLU, plus a second destination dst2 (+)= dz: the BatchNorm term and
 * the residual/identity term of one sum (pose_hrnet.py:54-55) share dz and are written in one pass */
int hrnet_grad_term2(int dtype, void* dst, void* dst2, const void* g, const void* mask_out, const void* y,
                     const float* scale, const float* shift, const float* coef, int N, int H, int W, int C,
                     int accumulate, int accumulate2, hr_stream_t stream);
/* partials[blocks][2][C]: sum(dz), sum(dz*y) with dz as above; blocks = hrnet_reduce_blocks() */
int hrnet_bn_bwd_reduce(int dtype, float* partials, const void* g, const void* mask_out,
                        const void* y, const float* scale, const float* shift, int N, int H, int W,
                        int C, int sh, int inner_relu, hr_stream_t stream);
hr_value_t hrnet_reduce_blocks(int N, int H, int W, int C);
/* dgamma/dbeta (+=) and coef[3][C]: A = gamma*invstd, B = -gamma*invstd^2*mean(dz*xhat)/... */
int hrnet_bn_bwd_finalize(const float* partials, int blocks, int C, float count,
                          const float* gamma, const float* save_mean, const float* save_invstd,
                          float* dgamma, float* dbeta, float* coef, int accumulate,
                          hr_stream_t stream);

/*
 * Head input: cat[N,H,W,sum(C_j)] = [x0, bilinear(x1), bilinear(x2), bilinear(x3)]
 * (F.upsample(mode='bilinear'), align_corners=False, then torch.cat: pose_hrnet.py:560-565;
 * align_corners=1: F.interpolate(..., align_corners=True) of pose_hrnet_softmax.py:499-503).
 * Branch j has spatial size (H>>j, W>>j) ... given explicitly. nbr <= 4.
 */
int hrnet_bilinear_cat(int dtype, void* cat, HR_HOST const void* const* xs, HR_HOST const int* hs,
                       HR_HOST const int* ws, HR_HOST const int* cs, int nbr, int N, int H, int W, int align_corners,
                       hr_stream_t stream);
/* dxs[j] (+)= bilinear^T(dcat[..., slice_j]) (gather form, deterministic) */
int hrnet_bilinear_cat_bwd(int dtype, const void* dcat, HR_HOST void* const* dxs, HR_HOST const int* hs,
                           HR_HOST const int* ws, HR_HOST const int* cs, int nbr, int N, int H, int W,
                           int align_corners, int accumulate, hr_stream_t stream);

/*
 * The head without its concat (pose_hrnet.py:560-566: F.upsample x3, torch.cat, last_layer[0] = Conv2d(480, 480, 1)).
 * A 1x1 convolution commutes with bilinear upsampling, so
 *     last_layer[0](cat(x0, up(x1), up(x2), up(x3))) = W0 x0 + up(W1 x1) + up(W2 x2) + up(W3 x3) + bias,
 * W_j = the columns of the weight that multiply branch j. The products t_j = W_j x_j are plain hrnet_conv2d launches
 * at branch j's resolution; hrnet_head_mix forms W0 x0 on the full-resolution grid, adds the bias and the bilinear
 * upsampling of t_1..t_nup (align_corners as hrnet_bilinear_cat), stores y once and gathers its batch statistics:
 *   rows_mode 0: stats = sums[8][2][Cout] (float atomics, as hrnet_conv2d with stats_atomic)
 *   rows_mode 1: stats = rows[hrnet_head_mix_rows(N,H,W)][2][Cout], one row per workgroup (deterministic)
 * bf16 (MFMA; C0 a multiple of 16, <= 128) or f32 (plain FMAs: the validation path), Cout <= 512 (hrnet_head_mix_supported).
 * w0: hrnet_pack_weights layout [Cout][C0].
 */
int hrnet_head_mix(int dtype, const void* x0, const void* w0, const float* bias, void* y, float* stats, int rows_mode,
                   HR_HOST const void* const* ts, HR_HOST const int* hs, HR_HOST const int* ws, int nup, int N, int H,
                   int W, int C0, int Cout, int align_corners, hr_stream_t stream);
hr_value_t hrnet_head_mix_rows(int N, int H, int W);
hr_value_t hrnet_head_mix_supported(int dtype, int C0, int Cout);
/* Backward of the 1x1 layer BEHIND the head's BatchNorm + ReLU (last_layer[3] of pose_hrnet.py:341-346) fused with that
 * BatchNorm's backward (autograd of nn.Conv2d / nn.ReLU / nn.BatchNorm2d): dz = wT dY (K = the layer's padded output
 * channels) is formed per pixel tile and masked by [bn_scale*y + bn_shift > 0] (inner_relu), never stored.
 *   mode 1: out = rows[hrnet_head_mix_rows(N,H,W)][2][Cout] f32, (sum dz, sum dz*y) per pixel tile (deterministic)
 *   mode 2: out = G[N,H,W,Cout] = A*dz + B*y + C with coef = [3][Cout] from hrnet_bn_bwd_finalize on those rows
 * wT: hrnet_pack_weights mode 1 of the layer's weight ([Cout][K]). Shapes as hrnet_head_mix_supported(dtype, K, Cout). */
int hrnet_head_bwd(int dtype, int mode, const void* dy, const void* wT, const void* y, void* out, const float* bn_scale,
                   const float* bn_shift, const float* coef, int inner_relu, int N, int H, int W, int K, int Cout,
                   hr_stream_t stream);
/* outs[k][N,hs[k],ws[k],C] = bilinear^T(G[N,H,W,C]) over ALL channels, k < nout <= 3: the gradients of t_j above
 * (autograd of F.upsample, pose_hrnet.py:561-563). Deterministic. Integer scales 2 / 4 / 8 with align_corners=0 take
 * ONE pass over G for all outputs (LDS-staged tiles); anything else (or streamed=1) a separable streamed walk per output. */
int hrnet_upsample_bilinear_t(int dtype, const void* g, HR_HOST void* const* outs, HR_HOST const int* hs,
                              HR_HOST const int* ws, int nout, int N, int H, int W, int C, int align_corners,
                              int streamed, hr_stream_t stream);

/* stem: NCHW f32 image -> im2col rows [N,Ho,Wo,Kpad] (k = (r*3+s)*C + c), 3x3 stride 2 pad 1
 * (conv1, pose_hrnet.py:283-284,512). */
int hrnet_im2col_stem(int dtype, const float* img_nchw, void* cols, int N, int C, int H, int W,
                      int Ho, int Wo, int Kpad, hr_stream_t stream);
/* [N,H,W,Cp] dtype -> [N,C,H,W] f32 (first C channels), and back (pad channels zeroed). */
int hrnet_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int H, int W, int Cp, int C,
                       hr_stream_t stream);
int hrnet_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int H, int W, int Cp, int C,
                       hr_stream_t stream);
/* dbias[c] (+)= sum over pixels of dy[pixels, Cp] for c < C (conv bias, pose_hrnet.py:334-347);
 * scratch: hrnet_reduce_blocks(1,1,pixels,Cp) * Cp floats */
int hrnet_bias_grad(int dtype, const void* dy, float* dbias, float* scratch, int pixels, int Cp,
                    int C, int accumulate, hr_stream_t stream);
int hrnet_fill_zero(void* p, int64_t bytes, hr_stream_t stream);

/*
 * HeatmapLoss (lib/core/loss.py:19-28): loss = mean_{b,k} sum_{h,w} (pred-gt)^2 (mode 0)
 * or |pred-gt| (mode 1). pred/gt are NCHW f32 [B,K,H,W] (the module contract).
 * partial: [B*K] f32 scratch; loss: [1] f32.
 */
int hrnet_heatmap_loss_fwd(const float* pred, const float* gt, float* partial, float* loss, int BK,
                           int HW, int mode, hr_stream_t stream);
/* dpred = gout * d loss / d pred */
int hrnet_heatmap_loss_bwd(const float* pred, const float* gt, const float* gout, float* dpred,
                           int BK, int HW, int mode, hr_stream_t stream);

/*
 * get_final_preds (lib/utils/heatmap_decoding.py:87-107), hms NCHW f32 [B,K,H,W] -> preds [B,K,2].
 *   expectation (use_softmax=True): (sum x*h, sum y*h), pixel coordinates, no normalisation
 *   argmax (use_softmax=False): first maximal flat index; u = idx % H, v = idx / H (H as the
 *   reference uses shape[2] for both)
 * maxvals (optional, [B,K]) receives the maximum (get_max_preds, lib/core/inference.py:18-46,
 * which uses W for % and / and zeroes preds whose max <= 0: flag `inference_style`).
 */
int hrnet_decode_expectation(const float* hms, float* preds, int BK, int H, int W,
                             hr_stream_t stream);
int hrnet_decode_expectation_bwd(const float* gpreds, float* dhms, int BK, int H, int W,
                                 int accumulate, hr_stream_t stream);
int hrnet_decode_argmax(const float* hms, float* preds, float* maxvals, int BK, int H, int W,
                        int inference_style, hr_stream_t stream);

/*
 * The data step either side of the path, on the device instead of the host loader:
 *   hrnet_gaussian_targets: lib/dataset/target_generators/target_generators.py:14-53 - un-normalised
 *     Gaussians, peak 1 at int(coord), window 6*sigma+3, zero map if invisible (visibility may be
 *     NULL = all visible) or out of range. pose2d [BK,2] heat-map pixels (x,y), heatmaps [BK,H,W].
 *   hrnet_normalize_u8: ToTensor + Normalize (lib/dataset/transforms/build.py:84-85): HWC u8 image
 *     -> CHW f32 (v/255 - mean[c]) / std[c]; mean3/std3 are HOST arrays of 3 floats.
 */
int hrnet_gaussian_targets(const float* pose2d, const float* visibility, float* heatmaps, int BK, int H,
                           int W, float sigma, hr_stream_t stream);
int hrnet_normalize_u8(const unsigned char* img_nhwc, float* out_nchw, int N, int H, int W,
                       HR_HOST const float* mean3, HR_HOST const float* std3, hr_stream_t stream);

/*
 * Input step of tools/inference.py (reference tools/inference.py:117-121: cv2.resize to IMAGE_SIZE, then
 * ToTensor + Normalize): a ragged batch of u8 HWC images in ONE device buffer of src_bytes bytes ->
 * out_nchw [n,3,Ho,Wo] f32. slots is a DEVICE table int64 [n][4] = {byte offset, H, W, row pitch (bytes)};
 * several rows may name the same bytes (PoseAggr frame windows). Resize: cv2 INTER_LINEAR geometry
 * (sx = (x+0.5)*W/Wo - 0.5, negative -> 0 with weight 0, x1 = min(x0+1, W-1); no antialiasing), the
 * blend in f32, rounded half to even and clamped to a u8 code, then (u/255 - mean[c]) / std[c] as
 * hrnet_normalize_u8 (bit-identical to it at Ho == H, Wo == W). Channel c is read from source channel
 * bgr ? 2-c : c. A row whose extent offset + (H-1)*pitch + 3*W exceeds src_bytes, or with H, W < 1 or
 * pitch < 3*W, is not read: its output plane is NaN. mean3/std3 are HOST arrays of 3 floats.
 */
int hrnet_resize_normalize_u8(const unsigned char* src, int64_t src_bytes, const int64_t* slots, int n,
                              float* out_nchw, int Ho, int Wo, HR_HOST const float* mean3, HR_HOST const float* std3,
                              int bgr, hr_stream_t stream);

/*
 * Training input step of the RHD reader (lib/dataset/rhd.py; reference RandomAffineTransform + RandomHorizontalFlip +
 * ToTensor + Normalize, lib/dataset/transforms/transforms.py:54-175): crops in ONE device buffer of src_bytes bytes
 * -> out_nchw [n,3,Ho,Wo] f32. slots is the DEVICE slot table of hrnet_resize_normalize_u8 (a crop is a slot whose
 * offset points at its top-left byte inside the image, with the image's row pitch); inv_mats is a DEVICE table
 * f32 [n][6]: the 2x3 inverse matrix (output pixel -> slot pixel, row-major) of each slot, flip folded in. Per
 * output pixel: the mapped position in f64, a bilinear blend in f32 in which each neighbour outside [0,W) x [0,H)
 * of the slot contributes 0 (cv2 BORDER_CONSTANT 0), rounded half to even and clamped to a u8 code, then
 * (u/255 - mean[c]) / std[c] as hrnet_normalize_u8 (bit-identical to it for an identity matrix at Ho == H,
 * Wo == W). A row outside the buffer, or with H, W < 1 or pitch < 3*W, is not read: its output plane is NaN.
 * mean3/std3 are HOST arrays of 3 floats.
 */
int hrnet_affine_warp_normalize_u8(const unsigned char* src, int64_t src_bytes, const int64_t* slots,
                                   const float* inv_mats, int n, float* out_nchw, int Ho, int Wo,
                                   HR_HOST const float* mean3, HR_HOST const float* std3, hr_stream_t stream);

/*
 * Multi-view DLT triangulation of tools/evaluate_3D.py (reference tools/evaluate_3D.py:178-190,270-301,
 * lib/models/triangulation_model_utils/multiview.py:120-187, lib/utils/misc.py:64-97), one thread per (sample, joint):
 *   pts       [B,V,K,2] f32, slot b*V + v (the order hrnet_decode_* leaves for a (B*V, K, H, W) heat-map batch)
 *   to_frame  [B*V,2,3] f64 or NULL: affine heat-map pixel -> frame pixel applied first; NULL: pts are frame pixels
 *   proj      [B,V,3,4] f64: K [R|t]
 *   conf      [B,V,K] f32 or NULL: a view's two rows are scaled by its weight (multiview.py:142-169)
 *   X         [B,K,3] f32: right singular vector of the 2V x 4 DLT matrix for its smallest singular value,
 *             v[0:3] / v[3], in f64 (Givens QR of the rows + one-sided Jacobi SVD; A^T A is never formed)
 *   pts_frame [B,V,K,2] f32 or NULL: the mapped 2-D points
 * 2 <= V <= 8. Fewer than two views of nonzero weight give NaN, v[3] = 0 a non-finite X.
 */
int hrnet_triangulate(const float* pts, const double* to_frame, const double* proj, const float* conf, float* X,
                      float* pts_frame, int B, int V, int K, hr_stream_t stream);

/*
 * Backward of hrnet_triangulate for the 3-D training loss (the reference back-propagates through torch.svd,
 * lib/models/triangulation_model_utils/multiview.py:142-169). pts, to_frame, proj, conf and B, V, K are the forward's
 * inputs, unchanged; nothing else is saved: the f64 Givens QR + Jacobi SVD is recomputed with the forward's device
 * code, which yields all four right singular vectors v_j and squared singular values n_j (A^T A is never formed).
 *   gX    [B,K,3] f32: dL/dX
 *   dpts  [B,V,K,2] f32: dL/d pts, the GIVEN points (through the 2 x 2 part of to_frame when there is one)
 *   dconf [B,V,K] f32 or NULL: dL/d conf (for conf NULL: with respect to a unit weight)
 * With h = v_m the forward's vector, g^ = [g / h3, -(g . h[0:3]) / h3^2] and z = -sum_{j != m} v_j (v_j . g^) /
 * (n_j - n_m): dL/dA = (A z) h^T + (A h) z^T, and for view v with weight c and rows a0 = x P[2] - P[0], a1 = y P[2] -
 * P[1]: dL/dx = c^2 ((a0 . z)(h . P[2]) + (a0 . h)(z . P[2])), dL/dy the same with a1, dL/dc = 2 c ((a0 . z)(a0 . h) +
 * (a1 . z)(a1 . h)). One launch for any B, one thread per point, f32 in and out, f64 inside, 2 <= V <= 8.
 * A view of weight 0 gets dpts = 0 and dconf = 0 exactly. A point whose X is NaN in the forward (fewer than two views
 * of nonzero weight, or a non-finite input) gets NaN in every view of that point and nowhere else. A vanishing gap
 * n_j - n_m gives the huge or non-finite values of the formula, as the reference's SVD backward does: they are
 * returned, not clamped. Nothing traps.
 */
int hrnet_triangulate_bwd(const float* pts, const double* to_frame, const double* proj, const float* conf,
                          const float* gX, float* dpts, float* dconf, int B, int V, int K, hr_stream_t stream);

/*
 * RANSAC over the views, then the DLT of hrnet_triangulate over the chosen views (reference lib/utils/misc.py:178-240
 * with direct_optimization off, as RANSACTriangulationNet.forward calls it). pts, to_frame, proj, pts_frame and
 * B, V, K as in hrnet_triangulate; there are no weights.
 *   pairs     int32 view-index pairs, the hypotheses, chosen by the host (the kernel draws nothing):
 *             pairs_per_point == 0: [n_hyp,2], one table for all points; != 0: [B*K,n_hyp,2], point b*K + k
 *   epsilon   inlier threshold on HALF the pixel distance in the frame between a view's point and the reprojection
 *             of the two-view solution (the reference's `1 / 2 * sqrt(...)`, multiview.py:196): 25 means 50 px
 *   X         [B,K,3] f32: the DLT over the final set, its views in ascending order
 *   inliers   [B,K] int32: bit v is set when view v is in the final set
 * Per point the hypotheses are taken in table order: a two-view DLT of (i, j), the candidate set {i, j} + {v : err_v <
 * epsilon}, which replaces the current set only when it is strictly larger (the first largest set wins). A pair with
 * i == j or an index outside 0..V-1 is skipped; with no usable pair (or n_hyp == 0) the set is every view. A group of
 * lanes per point solves the hypotheses side by side; the result does not depend on the grouping. Every solve is the
 * f64 Givens QR + Jacobi SVD of hrnet_triangulate, so epsilon = +inf reproduces hrnet_triangulate bit for bit.
 * 2 <= V <= 8, 0 <= n_hyp <= 64, epsilon not NaN. A non-finite point (after to_frame) or projection matrix in ANY view
 * of a point makes its X NaN, although the rule alone would drop such a view (its error is never below epsilon): as
 * in hrnet_triangulate, a fault upstream is not hidden. The mask is then the one the rule gives.
 */
int hrnet_triangulate_ransac(const float* pts, const double* to_frame, const double* proj, const int* pairs, int n_hyp,
                             int pairs_per_point, double epsilon, float* X, int* inliers, float* pts_frame, int B,
                             int V, int K, hr_stream_t stream);

/*
 * Volumetric lifting (csrc/volumetric.hip). All tensors f32 in the reference's module contract: features [B,V,C,H,W],
 * volumes [B,C,X,Y,Z], coordinate volumes [B,X,Y,Z,3] (world coordinates of the voxel centres), projections [B,V,3,4].
 * Element offsets are 64-bit. Limits of all six entries: 1 <= V <= 8, B <= 65535, X*Y*Z <= 2^30, H*W <=
 * HR_VOLUME_MAX_MAP (a 64-bit fixed-point plane of the backward must fit the LDS), B*J <= 65535; anything else is
 * HR_E_BADARG.
 */
#define HR_VOL_SUM 0
#define HR_VOL_MAX 1
#define HR_VOL_SOFTMAX 2
#define HR_VOL_CONF 3
#define HR_VOLUME_MAX_MAP 16384 /* H*W of a feature map: 128 KB of LDS as 64-bit cells (96x72 is 6912) */
#define HR_VOLUME_SPLIT 32      /* workgroups per map of hrnet_volume_integrate*: `work` holds B*J*32*5 doubles */

/*
 * unproject_heatmaps (reference lib/models/triangulation_model_utils/op.py:99-168), one launch for any B and V.
 * Per voxel p and view v: q = P[b,v] [p,1]; the view is invalid where q.z <= 0 (a q.z of exactly 0 becomes 1 before
 * the divide, op.py:124); u = q.x/q.z, w = q.y/q.z. The sample position is the REFERENCE'S rule, not a pixel-exact
 * one: op.py:129-130 normalises gx = 2(u/H - 0.5), gy = 2(w/W - 0.5) with (H, W) = heatmap_shape - the divisors are
 * swapped - and F.grid_sample(align_corners=True) then reads column u (W-1)/H and row w (H-1)/W. Bilinear, zero
 * padding (a corner outside the map contributes 0); the sample is 0 where the view is invalid. The projection and the
 * split into cell and fractional weights are f64 from the f32 inputs, the blend and the aggregation f32.
 *   method HR_VOL_SUM: sum_v s_v; HR_VOL_MAX: the largest sample; HR_VOL_SOFTMAX: sum_v s_v softmax_v(s)_v over the V
 *   samples, zeros of invalid or out-of-image views included (op.py:158-164); HR_VOL_CONF: sum_v conf[b,v,c] s_v
 *   (op.py:152-153), conf [B,V,C] f32 (NULL otherwise), not normalised here.
 */
int hrnet_unproject_volume(const float* features, const float* proj, const float* coord, const float* conf,
                           float* volumes, int method, int B, int V, int C, int H, int W, int X, int Y, int Z,
                           hr_stream_t stream);

/*
 * Backward of hrnet_unproject_volume (the reference's autograd through op.py:99-168) from gV [B,C,X,Y,Z]: dfeatures
 * [B,V,C,H,W], overwritten, and dconf [B,V,C] for HR_VOL_CONF (NULL otherwise, or when not wanted). Positions and
 * samples are recomputed from the forward's inputs. A view's sample gets gV times: sum 1; max 1 for the first largest
 * view, 0 for the others; softmax x_v (1 + s_v - sum_u s_u x_u), x = softmax_v(s); conf the weight. The projection
 * matrices and the coordinate volume are constants (no gradient - a deviation: the reference's grid_sample would
 * reach the cuboid through its grid gradient). One launch; a workgroup owns (b, v, 1..4 channels), accumulates the
 * scatter in LDS planes in 64-bit fixed point with integer atomics and stores them with plain stores: the result is
 * the same bits on every run. A non-finite gV[b,c], conf or feature plane gives a NaN dfeatures plane.
 */
int hrnet_unproject_volume_bwd(const float* features, const float* proj, const float* coord, const float* conf,
                               const float* gV, float* dfeatures, float* dconf, int method, int B, int V, int C, int H,
                               int W, int X, int Y, int Z, hr_stream_t stream);

/*
 * integrate_tensor_3d_with_coordinates (reference lib/models/triangulation_model_utils/op.py:84-96) with the model's
 * `volumes * VOLUME_MULTIPLIER` folded in: vols [B,J,X,Y,Z], coord [B,X,Y,Z,3].
 *   softmax != 0: p = softmax(multiplier * vols) over the X*Y*Z voxels of each map (the map's maximum is subtracted);
 *   softmax == 0: p = relu(multiplier * vols), not normalised.
 * keypoints [B,J,3] = sum p coord; p [B,J,X,Y,Z]. f32 in and out; the maximum, the sum and the three moments are f64,
 * computed as HR_VOLUME_SPLIT partials per map and merged in index order (a call is bit-reproducible).
 * work: B*J*HR_VOLUME_SPLIT*5 doubles of device scratch, contents undefined afterwards. Two launches.
 * backward, from gK [B,J,3] and gP [B,J,X,Y,Z] or NULL (zero), with t_i = gK . coord_i + gP_i:
 *   softmax: dvols_i = multiplier p_i (t_i - sum_j p_j t_j); relu: dvols_i = multiplier [multiplier vols_i > 0] t_i.
 * p is the forward's output; coord is a constant.
 */
int hrnet_volume_integrate(const float* vols, const float* coord, float multiplier, int softmax, float* keypoints,
                           float* p, double* work, int B, int J, int X, int Y, int Z, hr_stream_t stream);
int hrnet_volume_integrate_bwd(const float* vols, const float* p, const float* coord, const float* gK, const float* gP,
                               float multiplier, int softmax, float* dvols, double* work, int B, int J, int X, int Y,
                               int Z, hr_stream_t stream);

/*
 * VolumetricCELoss (reference lib/core/loss.py:225-256): per (b,j) the voxel of coord[b] nearest gt[b,j] (f64
 * distances, the first of equal distances wins) -> idx [B,J] int32, the flat index x*Y*Z + y*Z + z;
 * loss[0] = sum_{b,j} validity[b,j] (-log(p[b,j,idx] + 1e-6)) / (B*J) - the divisor counts every joint, valid or not,
 * as the reference does - f64 inside, summed in a fixed order. coord [B,X,Y,Z,3], p [B,J,X,Y,Z], gt [B,J,3],
 * validity [B,J].
 * backward: dp [B,J,X,Y,Z] is zeroed (hrnet_fill_zero) and dp[b,j,idx] = -*gout validity / (p + 1e-6) / (B*J);
 * gout is a device scalar, idx the forward's.
 */
int hrnet_volumetric_ce_loss(const float* coord, const float* p, const float* gt, const float* validity, float* loss,
                             int* idx, int B, int J, int X, int Y, int Z, hr_stream_t stream);
int hrnet_volumetric_ce_loss_bwd(const float* p, const float* validity, const int* idx, const float* gout, float* dp,
                                 int B, int J, int X, int Y, int Z, hr_stream_t stream);

/*
 * V2V inference (reference lib/models/v2v.py; called from lib/models/triangulation.py:349,467): the 3-D convolutions
 * of the volumetric models, eval-mode forward, f32 only (HR_BF16 is refused; the dtype argument is there so that bf16
 * can be added without an ABI change). Activations are NDHWC f32, element offsets 64-bit; Cin % 4 == 0 and
 * Cout % 16 == 0, pad channels zero. Stream-ordered, no allocation, no host synchronisation, no atomics: a call is
 * bit-reproducible. No dynamic LDS, so no function attribute is touched and every entry may be captured at once.
 *
 * conv3d: Conv3d(ks, stride 1, padding ks / 2), ks = 1 | 3 | 7 (v2v.py:11,24,27,35,160), any N, D, H, W >= 1, on the
 *   exact-f32 MFMA. w_packed [ks^3][Cout][Cin] from pack_weights3d. Epilogue on the f32 accumulator, in this order:
 *   acc * scale[c] + shift[c] (one fmaf; scale NULL = 1), + res[n,d,h,w,c] if res != NULL, ReLU if relu != 0: the
 *   eval-mode BatchNorm3d (v2v.py:12,25,28,36) with scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale
 *   built by the host in f64, the relu(res + skip) of Res3DBlock (v2v.py:39-42), and the bare output layer (shift = bias).
 * pack_weights3d: Conv3d's OIDHW [Cout][Cin][ks][ks][ks], or with transposed != 0 ConvTranspose3d's IODHW
 *   [Cin][Cout][ks][ks][ks], to [ks^3][Cout_pad][Cin_pad] with zeros in the pads. ks = 2 is the deconvolution's.
 * maxpool3d: F.max_pool3d(x, 2, 2) (v2v.py:50-51): y [N,D/2,H/2,W/2,C]; D, H and W must be even (HR_E_BADARG if not),
 *   C % 4 == 0.
 * deconv3d_k2s2: ConvTranspose3d(k = 2, s = 2) (v2v.py:60): x [N,D,H,W,Cin] -> y [N,2D,2H,2W,Cout],
 *   y[n,2d+a,2h+b,2w+c,:] = W[:,:,a,b,c]^T x[n,d,h,w,:]; w_packed [8][Cout][Cin]. Epilogue: acc * scale + shift, ReLU if
 *   relu != 0, THEN + add[n,.,.,.,c] if add != NULL - the decoder's x = upsample(x) + skip_x (v2v.py:123-136).
 * conv3d_supported: 1 if conv3d serves (dtype, Cin, Cout, ks), else 0. Pure host query, no error code.
 */
hr_value_t hrnet_conv3d_supported(int dtype, int Cin, int Cout, int ks);
int hrnet_conv3d(int dtype, const void* x, const void* w_packed, const float* scale, const float* shift,
                 const void* res, void* y, int N, int D, int H, int W, int Cin, int Cout, int ks, int relu,
                 hr_stream_t stream);
int hrnet_pack_weights3d(int dtype, const float* w, void* out, int Cout, int Cin, int ks, int Cout_pad, int Cin_pad,
                         int transposed, hr_stream_t stream);
int hrnet_maxpool3d(int dtype, const void* x, void* y, int N, int D, int H, int W, int C, hr_stream_t stream);
int hrnet_deconv3d_k2s2(int dtype, const void* x, const void* w_packed, const float* scale, const float* shift,
                        const void* add, void* y, int N, int D, int H, int W, int Cin, int Cout, int relu,
                        hr_stream_t stream);

/*
 * V2V training (csrc/conv3d_train.hip): what a training step of V2V needs beside the entries above. Same layout and
 * rules: NDHWC f32, 64-bit element offsets, Cin % 4 == 0, Cout % 16 == 0, pad channels zero on the way in and kept zero
 * on the way out, f32 only. Stream-ordered, no allocation, no host synchronisation, NO atomics: every sum has one
 * fixed order (per-workgroup or per-split partials in caller scratch, added in index order by a second launch), so a
 * call is bit-reproducible. Every argument check comes before the first launch. rows = N * D * H * W throughout.
 * The raw convolution output z of a training layer is hrnet_conv3d with scale = NULL, shift = bias, no res, no ReLU.
 *
 * bn3d_parts: the number P of partial rows the BatchNorm entries use for `rows` rows (at most 256); 0 for rows < 1.
 * bn3d_stats: training-mode BatchNorm3d statistics of z [rows][C]: mean, biased variance -> invstd = 1/sqrt(var + eps),
 *   scale = gamma * invstd, shift = beta - mean * scale (gamma / beta NULL = 1 / 0), all [C]. Two passes, sum z and then
 *   sum (z - mean)^2, never E[z^2] - E[z]^2. running_mean / running_var (both or neither; the first Creal channels)
 *   are updated with `momentum`, the variance unbiased (rows / (rows - 1)); *num_batches_tracked += 1 if not NULL.
 *   rows >= 2 (HR_E_BADARG with torch's "Expected more than 1 value per channel when training" otherwise);
 *   C <= 1024. scratch: 2 * P * C floats.
 * bn3d_apply: y = z * scale + shift (one fmaf); other_after_relu == 0: + other, then ReLU if relu (Res3DBlock);
 *   other_after_relu != 0: ReLU if relu, then + other (the decoder's upsample + skip). other may be NULL.
 * bn3d_bwd: with g = dy where the forward's ReLU passed (mask_y != NULL: where the saved output mask_y > 0;
 *   recompute_mask != 0: where fmaf(z, scale, shift) > 0, for a layer that added something AFTER its ReLU; neither: no
 *   ReLU) and xhat = (z - mean) * invstd:  dz = scale * (g - mean(g) - xhat * mean(g * xhat)),  dgamma = sum g * xhat,
 *   dbeta = sum g,  dbias (the convolution's, under the BatchNorm) = 0: sum dz is scale * (sum g - rows * mean(g) -
 *   mean(g xhat) * sum xhat), whose first two terms cancel and whose sum xhat is zero by the definition of the batch
 *   mean. dother (NULL or [rows][C]) receives g, written or with accumulate_other added to: the gradient of a residual
 *   input. (The gradient of a tensor added after the ReLU is dy itself: no pass.) dgamma / dbeta / dbias: NULL = skip,
 *   the first Creal channels, added to with accumulate_params. z == NULL (a layer without BatchNorm): only
 *   dbias (+)= sum dy is formed; dz, dother, mask_y, dgamma, dbeta must be NULL. scratch: (2 * P + 2) * C floats.
 * maxpool3d_bwd: x [N,D,H,W,C] is the pool's saved input, dy [N,D/2,H/2,W/2,C]; dx gets dy at the FIRST maximum of each
 *   2x2x2 window in (d, h, w) scan order (strict >: an all-equal window sends it to element 0, as torch on the CPU) and
 *   zero elsewhere; with accumulate it is added to dx.
 * pack_weights3d_dgrad: Conv3d's OIDHW to [ks^3][Cin_pad][Cout_pad] with out[tap][ci][co] = w[co][ci][ks^3 - 1 - tap]:
 *   transposed and tap-reversed, so that hrnet_conv3d(dz, out, NULL, zeros, res, dx, ..., Cin := Cout_pad,
 *   Cout := Cin_pad, ks, 0) is the input gradient (+ res). Cin_pad is the output side there: a multiple of 16 (the
 *   first layer's 4 input channels come out as 16, of which the layout transpose keeps the real ones).
 * deconv3d_k2s2_dgrad: dx[n,d,h,w,ci] (+)= sum over (a,b,c), co of w[ci][co][a][b][c] * dz[n,2d+a,2h+b,2w+c,co];
 *   w_packed [8][Cin][Cout] = pack_weights3d(w, Cout := Cin, Cin := Cout, ks 2, transposed 0). N, D, H, W are dx's.
 * conv3d_wgrad_scratch: pure host query: *bytes of scratch and *nsplit voxel splits that conv3d_wgrad uses for this
 *   shape (N, D, H, W: the volume the kernel walks - the convolution's, or the deconvolution's INPUT volume), and, if
 *   split_voxels != NULL, the voxels of one split: split k owns voxels [k * split_voxels, (k + 1) * split_voxels),
 *   the last one what is left.
 * conv3d_wgrad: dw[co][ci][tap] (+)= sum_v dz[v,co] * x[v + tap,ci] (taps outside the volume contribute nothing), OIDHW
 *   [Cout_real][Cin_real][ks^3]; deconv != 0: dw[ci][co][tap] (+)= sum_v x[v,ci] * dz[2v + tap,co], IODHW, ks = 2,
 *   x [N,D,H,W,Cin], dz [N,2D,2H,2W,Cout]. The voxels are split over workgroups into nsplit partial sums in scratch,
 *   which a second launch adds in split order. accumulate != 0 adds to dw, else dw is overwritten.
 */
hr_value_t hrnet_bn3d_parts(long long rows);
int hrnet_bn3d_stats(int dtype, const void* z, const float* gamma, const float* beta, float* scratch, float* mean,
                     float* invstd, float* scale, float* shift, float* running_mean, float* running_var,
                     long long* num_batches_tracked, int N, int D, int H, int W, int C, int Creal, float momentum,
                     float eps, hr_stream_t stream);
int hrnet_bn3d_apply(int dtype, const void* z, const float* scale, const float* shift, const void* other, void* y, int N,
                     int D, int H, int W, int C, int relu, int other_after_relu, hr_stream_t stream);
int hrnet_bn3d_bwd(int dtype, const void* dy, const void* z, const void* mask_y, const float* scale, const float* shift,
                   const float* mean, const float* invstd, float* scratch, void* dz, void* dother, float* dgamma,
                   float* dbeta, float* dbias, int N, int D, int H, int W, int C, int Creal, int recompute_mask,
                   int accumulate_other, int accumulate_params, hr_stream_t stream);
int hrnet_maxpool3d_bwd(int dtype, const void* x, const void* dy, void* dx, int N, int D, int H, int W, int C,
                        int accumulate, hr_stream_t stream);
int hrnet_pack_weights3d_dgrad(int dtype, const float* w, void* out, int Cout, int Cin, int ks, int Cout_pad,
                               int Cin_pad, hr_stream_t stream);
int hrnet_deconv3d_k2s2_dgrad(int dtype, const void* dz, const void* w_packed, void* dx, int N, int D, int H, int W,
                              int Cin, int Cout, int accumulate, hr_stream_t stream);
int hrnet_conv3d_wgrad_scratch(int dtype, int N, int D, int H, int W, int Cin, int Cout, int ks, int deconv,
                               HR_HOST long long* bytes, HR_HOST int* nsplit, HR_HOST long long* split_voxels);
int hrnet_conv3d_wgrad(int dtype, const void* x, const void* dz, void* scratch, long long scratch_bytes, float* dw, int N,
                       int D, int H, int W, int Cin, int Cout, int Cin_real, int Cout_real, int ks, int deconv,
                       int accumulate, hr_stream_t stream);

/*
 * 1x1 convolution on NCHW f32 with the module's own weight, read in place (csrc/pointwise.hip): process_features of the
 * volumetric model (reference lib/models/triangulation.py:345-349). f32 only; P = H * W pixels per plane.
 *   forward:  y[n,o,p] = bias[o] + sum_c w[o,c] x[n,c,p]; x [N,Cin,P], w [Cout,Cin], bias [Cout] or NULL, y [N,Cout,P].
 *   backward: dx[n,c,p] = sum_o w[o,c] dy[n,o,p], dw[o,c] = sum_{n,p} dy[n,o,p] x[n,c,p], db[o] = sum_{n,p} dy[n,o,p];
 *             each of dx, dw, db may be NULL (not all three) and the others do not depend on which are. dw and db go
 *             through `scratch`: hrnet_pointwise_nchw_parts(N, P) rows of Cout * Cin + Cout floats, one per workgroup
 *             of the first launch, added in index order by a second one. scratch is needed only with dw or db.
 * hrnet_pointwise_nchw_supported: 1 for f32, 1 <= Cin <= 65536, 1 <= Cout <= 64. Further limits, refused: N <= 65535,
 * P <= 2^30, N * P * max(Cin, Cout) <= 2^40. hrnet_pointwise_nchw_parts: 0 for sizes outside these limits.
 * No atomics: a call is bit-reproducible. Any P, Cin and Cout within the limits; 16-byte accesses are used when
 * P % 4 == 0 (Cin % 4 == 0 for w) and the pointers are 16-byte aligned.
 */
hr_value_t hrnet_pointwise_nchw_supported(int dtype, int Cin, int Cout);
int hrnet_pointwise_nchw(int dtype, const float* x, const float* w, const float* bias, float* y, int N, int Cin,
                         int Cout, long long P, hr_stream_t stream);
hr_value_t hrnet_pointwise_nchw_parts(int N, long long P);
int hrnet_pointwise_nchw_bwd(int dtype, const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                             float* scratch, long long scratch_floats, int N, int Cin, int Cout, long long P,
                             hr_stream_t stream);

/*
 * Cross-view heat-map fusion of multiview_pose_hrnet (csrc/view_fusion.hip; reference
 * lib/models/multiview_pose_hrnet.py:57-71). H, F, dF, dH are [B][V][K][P] f32 (P = h * w); W and dW are HOST arrays of
 * V * (V - 1) device pointers, the way hrnet_sum_terms takes its sources; W[n] is the [P_out][P_in] weight of an
 * nn.Linear, read in place (nothing is packed or copied). n(i,j) = i * (V - 1) + (rank of j among the views != i).
 *   forward:  F[b,i,k,:] = w_self * H[b,i,k,:] + w_other * sum_{j != i} H[b,j,k,:] @ W[n(i,j)]^T        (one launch)
 *   backward: dH[b,j,k,:] = w_self * dF[b,j,k,:] + w_other * sum_{i != j} dF[b,i,k,:] @ W[n(i,j)]       (one launch)
 *             dW[n(i,j)] = w_other * dF[:,i]^T @ H[:,j], summed over the B * K rows                      (one launch)
 *             dH may be NULL (then W may be NULL too); dW may be NULL (then H may be NULL), and a NULL entry of dW
 *             skips that matrix. Not both NULL. Neither half needs scratch memory.
 * hrnet_view_fusion_supported: 1 for f32, 2 <= V <= 4, 1 <= P <= 2^20. Further limits, refused: B, K >= 1,
 * B * V * K * P < 2^31. No atomics: every sum has one fixed order, so a call is bit-reproducible. 16-byte accesses are
 * used when P % 4 == 0 and every pointer is 16-byte aligned; any other P takes element-wise loads in the same kernels.
 * A weight element is read once per forward and once per dH pass while B * K <= 192; each dW element is written once.
 */
hr_value_t hrnet_view_fusion_supported(int dtype, int V, int P);
int hrnet_view_fusion(int dtype, const float* H, HR_HOST const void* const* W, float* F, int B, int V, int K, int P,
                      float w_self, float w_other, hr_stream_t stream);
int hrnet_view_fusion_bwd(int dtype, const float* H, HR_HOST const void* const* W, const float* dF, float* dH,
                          HR_HOST void* const* dW, int B, int V, int K, int P, float w_self, float w_other,
                          hr_stream_t stream);

/*
 * Transformer kernels of pose_hrnet_transformer, the reference's PoseFormer head (csrc/transformer.hip; reference
 * lib/models/pose_hrnet_transformer.py:21-85, :195-221). Everything is f32, row-major (rows, C), 64-bit element
 * offsets; an nn.Linear weight (Cout, Cin) is read in place. No float atomics: every sum has one fixed order, so a call
 * is bit-reproducible. Every entry refuses what it has no kernel for (HR_E_BADARG) before it launches anything.
 *
 * The query, hrnet_tf_supported, takes (op, a, b): HR_TF_LAYERNORM (C, unused), HR_TF_LINEAR (Cin, Cout), both up to
 * 65536; HR_TF_ATTENTION (N, hd): 1 <= N <= 64 tokens, 1 <= hd <= 128; HR_TF_FRAME_MEAN (F, unused): 1 <= F <= 65534.
 * Rows: 1 .. 2^22.
 *
 * LayerNorm over the last axis: y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance. The backward recomputes
 * the statistics from x and gives dx, dgamma, dbeta (each may be NULL, not all); the column sums are a two-stage
 * reduction through `scratch`, at least the number of floats the scratch query returns for (rows, C), needed only with
 * dgamma or dbeta.
 *
 * Linear: y = [res +] row_scale[row] * act(x W^T + bias). bias, res (rows, Cout), row_scale (rows) may be NULL. act:
 * HR_TF_ACT_NONE or HR_TF_ACT_GELU (exact, the erf form). With GELU and `pre` not NULL the pre-activation x W^T + bias
 * is stored there: the backward TAKES it as an input. Backward: g = dy * row_scale[row] * act'(pre);
 * dx = g W, dW = g^T x, db = column sums of g; each may be NULL (not all), x may be NULL without dW, W without dx. The
 * gradient of res is dy itself. Products run on mfma_f32_16x16x4f32; 16-byte accesses when Cin % 4 == 0, Cout % 4 == 0
 * and the pointers are 16-byte aligned, element-wise loads in the same kernels otherwise (Cin = 2, Cout = 42).
 *
 * Attention on a packed qkv (S, N, 3, heads, hd): out (S, N, heads * hd) = softmax(q k^T * scale) v per (sequence,
 * head), one wave each; scores and probabilities stay in LDS. The backward recomputes the probabilities from qkv and
 * gives dqkv; nothing else is saved.
 *
 * Frame mean: y[s, :] = sum_f w[f] * x[s, f, :] + b[0] (b may be NULL), x (S, F, D). Backward: dx, dw (F), db (1), each
 * may be NULL (not all).
 *
 * Add rows: y[r, :] = x[r, :] + pos[r % period, :], pos (period, C). Its backward is the identity for x
 * and the frame mean with unit weights for pos.
 */
enum { HR_TF_LAYERNORM = 0, HR_TF_LINEAR = 1, HR_TF_ATTENTION = 2, HR_TF_FRAME_MEAN = 3 };
enum { HR_TF_ACT_NONE = 0, HR_TF_ACT_GELU = 1 };
hr_value_t hrnet_tf_supported(int op, int a, int b);
long long hrnet_tf_layernorm_scratch(long long rows, int C);
int hrnet_tf_layernorm(const float* x, const float* gamma, const float* beta, float* y, long long rows, int C, float eps,
                       hr_stream_t stream);
int hrnet_tf_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta,
                           float* scratch, long long scratch_floats, long long rows, int C, float eps,
                           hr_stream_t stream);
int hrnet_tf_linear(const float* x, const float* W, const float* bias, const float* res, const float* row_scale,
                    float* y, float* pre, long long rows, int Cin, int Cout, int act, hr_stream_t stream);
int hrnet_tf_linear_bwd(const float* x, const float* W, const float* dy, const float* pre, const float* row_scale,
                        float* dx, float* dW, float* db, long long rows, int Cin, int Cout, int act,
                        hr_stream_t stream);
int hrnet_tf_attention(const float* qkv, float* out, int S, int N, int heads, int hd, float scale, hr_stream_t stream);
int hrnet_tf_attention_bwd(const float* qkv, const float* dout, float* dqkv, int S, int N, int heads, int hd,
                           float scale, hr_stream_t stream);
int hrnet_tf_frame_mean(const float* x, const float* w, const float* b, float* y, long long S, int F, long long D,
                        hr_stream_t stream);
int hrnet_tf_frame_mean_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                            long long S, int F, long long D, hr_stream_t stream);
int hrnet_tf_add_rows(const float* x, const float* pos, float* y, long long rows, int C, int period,
                      hr_stream_t stream);

/*
 * Swin kernels of swin_transformer, the reference's SwinPose (csrc/swin.hip; reference lib/models/swin_transformer.py).
 * Everything is f32, row-major, 64-bit element offsets, no float atomics: a call is bit-reproducible. Every
 * entry refuses what it has no kernel for (HR_E_BADARG) before it launches anything. The query takes (op, a, b):
 * HR_SWIN_ATTENTION (ws, hd): 1 <= ws * ws <= 64, 1 <= hd <= 128; HR_SWIN_MERGE (C, unused): 1 <= 4 C <= 65536;
 * HR_SWIN_EMBED (Cin, p): 1 <= Cin * p * p <= 65536.
 *
 * Window attention straight from token order (:237-269, :317-368, :491-510): qkv (B, H * W, 3, heads, hd) as the qkv linear
 * wrote it for the UNPADDED tokens, qkv_bias (3 * heads * hd), bias_table ((2 ws - 1)^2, heads), out (B, H * W, heads * hd).
 * Hp, Wp = H, W rounded up to multiples of ws. A token of the padded border has q = k = v = the qkv bias (the reference
 * pads after norm1 and before the qkv linear); it takes part as key and query, its output row is dropped. With shift > 0
 * token (i, j) of the shifted grid is padded-grid token ((i + shift) mod Hp, (j + shift) mod Wp), and -100 is added to the
 * logit of two tokens whose region ids 3 * band(i, Hp) + band(j, Wp) differ (bands [0, Hp - ws), [Hp - ws, Hp - shift),
 * [Hp - shift, Hp)). logit = scale * q.k + bias_table[rel(n, m), head], rel = the reference's relative_position_index.
 * One workgroup per (image, window, head); q, k, v, logits and probabilities live in LDS; both products run on
 * mfma_f32_16x16x4f32 with the ws * ws tokens padded to 64 (a padding lane's probability is exactly 0).
 *
 * Patch merging + LayerNorm (:390-415): x (B, H, W, C) -> y (B * ceil(H / 2) * ceil(W / 2), 4 C), channel blocks
 * [x(0,0), x(1,0), x(0,1), x(1,1)] (row parity fastest), zeros beyond an odd H or W, then LayerNorm(4 C) with f64 row
 * sums. gamma and beta both NULL: the gathered rows are stored as they are (no LayerNorm).
 *
 * Patch rows (:550-559): NCHW x (B, Cin, H, W) -> rows (B * ceil(H / p) * ceil(W / p), Cin * p * p), column
 * c * p * p + kh * p + kw, zeros right of W and below H: a Conv2d(Cin, E, p, stride p) weight (E, Cin, p, p) is then the
 * (E, Cin * p * p) matrix of a plain linear launch, read in place.
 */
enum { HR_SWIN_ATTENTION = 0, HR_SWIN_MERGE = 1, HR_SWIN_EMBED = 2 };
hr_value_t hrnet_swin_supported(int op, int a, int b);
int hrnet_swin_attention(const float* qkv, const float* qkv_bias, const float* bias_table, float* out, int B, int H,
                         int W, int heads, int hd, int ws, int shift, float scale, hr_stream_t stream);
int hrnet_swin_merge_ln(const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C,
                        float eps, hr_stream_t stream);
int hrnet_swin_patch_rows(const float* x, float* rows, int B, int Cin, int H, int W, int p, hr_stream_t stream);

/*
 * Backward of the Swin kernels (csrc/swin.hip), for training SwinPose. Same ranges and argument checks as the forward
 * entries, each before the first launch.
 *
 * Window attention backward: from qkv, qkv_bias, bias_table (as the forward took them) and dout (B, H * W, heads * hd) it
 * recomputes S = scale q k^T + table[rel] + mask and P = softmax(S) per (image, window, head) - nothing is saved by the
 * forward - and gives dV = P^T dO, dP = dO v^T, dS = P (dP - rowsum(P dP)), dq = scale dS k, dk = scale dS^T q; the -100
 * mask is a constant. dqkv (B, H * W, 3, heads, hd): a real token lies in one window, its row is written once. A token of
 * the padded border has q = k = v = the qkv bias: as a key its dk and dv go to dqkv_bias (3 * heads * hd), the k and v
 * thirds, head h's slice; as a query its output row was dropped, so its dO row, its dS row and its dq are exactly zero and
 * the q third of dqkv_bias is written as zeros. dqkv_bias is the attention's own contribution only (all zeros when no token
 * is padded); the qkv linear's bias gradient is separate. dtable ((2 ws - 1)^2, heads): dtable[rel(n, m), h] = the sum of
 * dS[n, m] over n, m < ws * ws (padded keys included), windows and images. dqkv_bias and dtable may each be NULL; with
 * either given, scratch (8-byte aligned) must hold hrnet_swin_attention_bwd_scratch(B, H, W, heads, hd, ws) floats =
 * 2 * workgroups * ((2 ws - 1)^2 + 2 hd): each workgroup sums its dS into the bins (one thread per bin) and its padded
 * keys' dk, dv in a fixed order into its own row, and a second launch adds the rows per head in workgroup order. Those
 * sums are f64 throughout (a row holds f64 values, two floats each). The query is pure host code and returns 0 for a
 * shape the entry refuses (among them one whose rows would take more than 2^31 - 1 floats). dqkv must not alias qkv or dout; scratch must alias nothing.
 *
 * Merge scatter, the inverse of hrnet_swin_merge_ln with gamma = NULL: dy (B * ceil(H / 2) * ceil(W / 2), 4 C) ->
 * dx (B, H, W, C); every pixel lies in one row and block, gradients at the zero padding of an odd H or W are dropped.
 *
 * Patch rows backward, the inverse of hrnet_swin_patch_rows: drows (B * ceil(H / p) * ceil(W / p), Cin * p * p) ->
 * dx (B, Cin, H, W) NCHW; gradients at the padding right of W and below H are dropped.
 *
 * Deconvolution input gradient, for the decoder's ConvTranspose2d(Cin, Cout, 3, 2, 1, 1): du (B, 2 H, 2 W, Cout_p) NHWC ->
 * dx (B, H, W, Cin_p), dx[b, i, j, ci] = sum over taps and co of du[b, 2 i - 1 + kh, 2 j - 1 + kw, co] * w[ci, co, kh, kw],
 * w_packed = hrnet_pack_weights(mode 0) of the weight read as OIHW (Cin, Cout, 3, 3): [Cin_p][9][Cout_p]. It is the
 * stride-2 3x3 convolution that hrnet_conv2d also computes; this entry exists for its summation: the 9 * Cout_p terms
 * (3456 at 384 channels) are added in f64 from 32-term f32 MFMA chunks, where the convolution entry's single f32 chain
 * misses the training tests' error rule at 768 -> 384 channels. Cout_p, Cin_p multiples of 4.
 */
hr_value_t hrnet_swin_attention_bwd_scratch(int B, int H, int W, int heads, int hd, int ws);
int hrnet_swin_attention_bwd(const float* qkv, const float* qkv_bias, const float* bias_table, const float* dout,
                             float* dqkv, float* dqkv_bias, float* dtable, float* scratch, long long scratch_floats,
                             int B, int H, int W, int heads, int hd, int ws, int shift, float scale, hr_stream_t stream);
int hrnet_swin_merge_scatter(const float* dy, float* dx, int B, int H, int W, int C, hr_stream_t stream);
int hrnet_swin_patch_rows_bwd(const float* drows, float* dx, int B, int Cin, int H, int W, int p, hr_stream_t stream);
int hrnet_swin_deconv_dgrad(const float* du, const float* w_packed, float* dx, int B, int H, int W, int Cout_p, int Cin_p,
                            hr_stream_t stream);

/*
 * NMF kernels of pose_hrnet_hamburger, the reference's HamNet (csrc/nmf.hip; reference lib/models/hamburger/ham.py, NMF2D
 * :227-269 on _MatrixDecomposition2DBase :14-117). Everything is f32, 64-bit element offsets, no float atomics: every sum
 * has one fixed order, so a call is bit-reproducible. Products run on mfma_f32_16x16x4f32; any size >= 1, edge tiles are
 * bounds-checked in the kernel; an operand is read with 16-byte accesses when its pointer is 16-byte aligned and its
 * leading dimension and batch stride are multiples of 4, with element-wise loads in the same kernel otherwise. Every entry
 * refuses what it has no kernel for (HR_E_BADARG) before it launches anything. The query takes (op, a, b): HR_NMF_UPDATE
 * (K, R), HR_NMF_GRAM (K, R), HR_NMF_PRODUCT (K, R): each 1 .. 2^24; batches G: 1 .. 65535.
 *
 * The feature matrix is never copied or transposed: an entry that reads it takes (x, ldx, bsx, xt) and reads
 * op(X)_g[i, k] = x[g * bsx + i * ldx + k] (xt = 0) or x[g * bsx + k * ldx + i] (xt = 1), so a channel half of a wider
 * NCHW or NHWC tensor and both orientations of a ham go through the same code. T, F, Gm and the results are dense
 * row-major, batch after batch.
 *
 * Update, the multiplicative step (:246-257): Tout = T * (op(X) F) / (T Gm + eps) for T, Tout (G, M, R), F (G, K, R),
 * op(X) (G, M, K), Gm (G, R, R). Both products of an output tile are accumulated in registers and the ratio is taken
 * there: neither reaches memory. Out of place (a tile's T Gm reads whole rows of T). Coefficients: (T, F, op(X)) =
 * (coef, bases, X^T) with Gm = bases^T bases; bases: (bases, coef, X) with Gm = coef^T coef.
 *
 * Gram: Gm (G, R, R) = A^T A for A (G, K, R). A long K is split over workgroups; the parts go through `scratch`, at least
 * hrnet_nmf_gram_scratch(G, K, R) floats (0 when nothing is split: scratch may then be NULL), and are added in split
 * order by a second launch. The query is pure host code and returns 0 for a shape the entry refuses (among them one whose
 * parts would take more than 2^31 - 1 floats).
 *
 * Product: out (G, M, R) = op(X) F, the logits of the initial softmax (:51; the row softmax itself is
 * hrnet_spatial_softmax_fwd on G * M rows of R). Reconstruct (:93): out_g[d, n] = sum_r Bs[d, r] Cf[n, r] for Bs (G, D, R),
 * Cf (G, N, R), stored at out[g * bso + d * ldo + n] (ot = 0) or out[g * bso + n * ldo + d] (ot = 1): a ham's result goes
 * straight into its channels of the next layer's input.
 */
enum { HR_NMF_UPDATE = 0, HR_NMF_GRAM = 1, HR_NMF_PRODUCT = 2 };
hr_value_t hrnet_nmf_supported(int op, int a, int b);
int hrnet_nmf_update(const float* T, const float* F, const float* x, long long ldx, long long bsx, int xt, const float* Gm,
                     float* Tout, int G, int M, int K, int R, float eps, hr_stream_t stream);
hr_value_t hrnet_nmf_gram_scratch(int G, int K, int R);
int hrnet_nmf_gram(const float* A, float* Gm, float* scratch, long long scratch_floats, int G, int K, int R,
                   hr_stream_t stream);
int hrnet_nmf_product(const float* x, long long ldx, long long bsx, int xt, const float* F, float* out, int G, int M, int K,
                      int R, hr_stream_t stream);
int hrnet_nmf_reconstruct(const float* Bs, const float* Cf, float* out, long long ldo, long long bso, int ot, int G, int D,
                          int N, int R, hr_stream_t stream);

/*
 * The burger's glue of pose_hrnet_hamburger in training mode (csrc/burger_train.hip; reference
 * lib/models/hamburger/burger.py:198-199 and the Dropout2d of lib/models/pose_hrnet_hamburger.py:62). Streaming kernels:
 * f32, NHWC rows [rows][C], C % 16 == 0, 64-bit element offsets (rows * C <= 2^40), pad channels zero on the way in and
 * kept zero on the way out. Stream-ordered, no allocation, no host synchronisation, NO atomics. Every argument check
 * (HR_E_BADARG) comes before the first launch. The grid is a fixed number of workgroups, a function of the shape alone,
 * that strides over the map; 16-byte accesses when every map pointer is 16-byte aligned, element-wise accesses in the same
 * kernel otherwise. The ham's own gradient needs no entry here: it is hrnet_nmf_update with dY where X sits, then
 * hrnet_nmf_reconstruct (lib/hipnet/nmf_train.py).
 *
 * burger_mix: out = relu(*coef_ham * u + *coef_shortcut * s). The two coefficients are device scalars: nothing is read on
 *   the host. out may be u itself (not s).
 * burger_mix_scratch: pure host query: the doubles of scratch the backward needs for this shape, 0 for a shape it refuses.
 * burger_mix_bwd: ONE pass over the maps. With gm = g where out > 0, else 0: du = *coef_ham * gm, ds = *coef_shortcut * gm
 *   (both WRITTEN; a caller that has more to add to ds accumulates into it afterwards, hrnet_conv2d's accumulate flag),
 *   dcoef[0] = sum gm * u, dcoef[1] = sum gm * s as floats. The sums are made in double: per thread, then per workgroup in
 *   a fixed order into scratch [workgroups][2], which a second launch adds in index order - a call is bit-reproducible.
 *   du may be g itself. du, ds, dcoef: NULL = not formed (at least one is given); scratch may be NULL when dcoef is.
 * dropout2d: y[b, p, c] = x[b, p, c] * keep[b * C + c], x and y [B][P][C], keep [B][C]: Dropout2d with the mask given (keep
 *   holds 0 or 1 / (1 - p)). y may be x itself. The same entry is its own backward (dx = dy * keep).
 */
int hrnet_burger_mix(const float* u, const float* s, const float* coef_ham, const float* coef_shortcut, float* out,
                     long long rows, int C, hr_stream_t stream);
hr_value_t hrnet_burger_mix_scratch(long long rows, int C);
int hrnet_burger_mix_bwd(const float* g, const float* out, const float* u, const float* s, const float* coef_ham,
                         const float* coef_shortcut, float* du, float* ds, float* dcoef, double* scratch,
                         long long scratch_doubles, long long rows, int C, hr_stream_t stream);
int hrnet_dropout2d(const float* x, const float* keep, float* y, int B, long long P, int C, hr_stream_t stream);

/*
 * Spatial softmax head of pose_hrnet_softmax (lib/models/pose_hrnet_softmax.py:520-524):
 * out[bk, :] = softmax(x[bk, :] * *temp) over the HW positions of each map, NCHW f32.
 * backward: dx = temp * out * (gout - sum(gout*out)); dtemp_partial[bk] = sum_i dz_i * x_i with
 * dz = out * (gout - sum(gout*out)) (the caller sums the BK partials: d loss / d temperature).
 */
int hrnet_spatial_softmax_fwd(const float* x, const float* temp, float* out, int BK, int HW,
                              hr_stream_t stream);
int hrnet_spatial_softmax_bwd(const float* x, const float* out, const float* gout, const float* temp,
                              float* dx, float* dtemp_partial, int BK, int HW, hr_stream_t stream);

/*
 * JointsMSELoss (lib/core/loss.py:37-50): sum_bk ||pred-gt||_2 * vis / max(1, sum vis), or
 * sum/K without visibility (vis NULL). pred/gt [B,K,2] f32, vis [B,K] f32.
 */
int hrnet_joints_loss_fwd(const float* pred, const float* gt, const float* vis, float* loss, int B,
                          int K, hr_stream_t stream);
int hrnet_joints_loss_bwd(const float* pred, const float* gt, const float* vis, const float* gout,
                          float* dpred, int B, int K, hr_stream_t stream);

/*
 * Joints3DMSELoss (lib/core/loss.py:137-148) of the 3-D training step: sum over batch and joints of
 * ||gt - pred||_2, over K - a sum over the batch, as the reference computes it. pred/gt [B,K,3] f32, loss[0] f32; f64
 * inside, summed in a fixed order (a call is bit-reproducible). backward: dpred = *gout / K * (pred - gt) /
 * ||pred - gt||, 0 for a zero difference (torch.norm backward); gout is a device scalar.
 */
int hrnet_joints3d_loss_fwd(const float* pred, const float* gt, float* loss, int B, int K, hr_stream_t stream);
int hrnet_joints3d_loss_bwd(const float* pred, const float* gt, const float* gout, float* dpred, int B, int K,
                            hr_stream_t stream);

/*
 * Hand-structure regularisers of the 2-D training step: BoneLengthLoss and JointAngleLoss (lib/core/loss.py:150-223)
 * on 2-D poses, optionally after scale_pose2d (lib/utils/transforms.py:146-175) of both poses. ONE launch for any B.
 *   pred, gt [B,21,2] f32 (gt may be NULL without the bone term); K must be 21;
 *   normalize != 0: r = p - p[0], then r / ||r[9] - r[0]|| per sample, no epsilon;
 *   terms: bit 0 bone length, bit 1 joint angle; outputs of a term that is off are not touched.
 *   loss_bone[0]  = sum over batch and j = 1..20 of (|gt[j]-gt[j-1]| - |pred[j]-pred[j-1]|)^2 / 20 (every j: the
 *                   bones 5-4, 9-8, 13-12, 17-16 included, as the reference computes them; a sum over the batch);
 *   loss_angle[0] = sum over batch and fingers f = 0..4 (joints 4f..4f+4, bone_i = x[4f+i] - x[4f+i-1]) of d^2 for
 *                   each d < 0 of d1 = (b4 x b3)(b3 x b2), d2 = (b2 x b1)(b3 x b2), u x v = u.x v.y - u.y v.x;
 *                   the coplanarity rule is exactly zero on z = 0 and enters only as the IEEE value the reference
 *                   gives it (0 for finite poses, NaN for non-finite ones);
 *   dbone_dpred, dangle_dpred [B,21,2] f32 or NULL: d loss / d pred (the UNSCALED pred, through the normalisation).
 * f32 in and out, f64 inside; the batch sum runs in sample order, so a call is bit-reproducible. A zero-length
 * predicted or ground-truth bone has no gradient (torch.norm backward); a zero scale makes both losses and that
 * sample's gradients non-finite, as in the reference - they are returned, nothing traps.
 * hrnet_structure_loss_bwd: dpred = *g_bone * dbone_dpred + *g_angle * dangle_dpred, one launch; g_* are device
 * scalars, a NULL one drops its term (at least one is given).
 */
int hrnet_structure_loss(const float* pred, const float* gt, float* loss_bone, float* loss_angle,
                         float* dbone_dpred, float* dangle_dpred, int B, int K, int normalize, int terms,
                         hr_stream_t stream);
int hrnet_structure_loss_bwd(const float* dbone_dpred, const float* dangle_dpred, const float* g_bone,
                             const float* g_angle, float* dpred, int B, int K, hr_stream_t stream);

/* Adam step over a flat f32 parameter buffer (torch.optim.Adam semantics incl. L2 weight
 * decay added to the gradient; lib/utils/utils.py:81-85, lib/core/function.py:101-106). */
int hrnet_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    float grad_scale, hr_stream_t stream);

/*
 * Deformable convolution v1 (lib/deformable_conv/functions/deform_conv_func.py:18-66, which binds
 * DCN.deform_conv_forward / deform_conv_backward of src/cuda/deform_conv_cuda.cu:19,139; sampling
 * rule src/cuda/deform_im2col_cuda.cuh:24-189). All tensors NCHW f32:
 *   input [B,C,H,W], offset [B, deformable_groups*2*kh*kw, Ho, Wo] (per tap: dy plane, dx plane),
 *   weight [Co, C/groups, kh, kw], bias [Co] or NULL, output [B,Co,Ho,Wo].
 * No column buffer is materialised, so the reference's im2col_step has no counterpart here (any
 * value gives the same result - the reference's own invariant, test.py:218-248).
 * backward: grad_input is accumulated with float atomics like the reference's col2im (zeroed
 * inside) - except on the PoseAggr geometry (one input channel per deformable group, groups = 1, 3x3,
 * Co <= 28, planes that fit LDS), whose single-pass kernel sums it in a 64-bit fixed-point plane: the
 * exact sum of the f32 contributions, the same bits on every run; grad_bias may be NULL; scratch holds hrnet_deform_conv_wgrad_blocks() *
 * (Co/groups)*(C/groups)*kh*kw floats. Limits: Co/groups <= 64 for backward, weight slice of one
 * group <= 96 KB.
 */
int hrnet_deform_conv_forward(const float* input, const float* offset, const float* weight,
                              const float* bias, float* output, int B, int C, int H, int W, int Co,
                              int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int groups, int deformable_groups, hr_stream_t stream);
hr_value_t hrnet_deform_conv_wgrad_blocks(int B, int Ho, int Wo);
int hrnet_deform_conv_backward(const float* input, const float* offset, const float* weight,
                               const float* grad_output, float* grad_input, float* grad_offset,
                               float* grad_weight, float* grad_bias, float* scratch, int B, int C,
                               int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                               int dh, int dw, int groups, int deformable_groups,
                               hr_stream_t stream);

/* Modulated deformable convolution (DCNv2): the same op with every sample multiplied by
 * mask [B, deformable_groups*kh*kw, Ho, Wo]. Replaces DCN.modulated_deform_conv_forward / _backward bound by
 * lib/deformable_conv/functions/modulated_deform_conv_func.py:25-33,44-56 (src/modulated_deform_conv.h:10-86,
 * src/cuda/modulated_deform_conv_cuda.cu:20-285, kernels src/cuda/modulated_deform_im2col_cuda.cuh:128-330).
 * backward: grad_input is zeroed inside; grad_mask like mask; scratch as for hrnet_deform_conv_backward. */
int hrnet_modulated_deform_conv_forward(const float* input, const float* offset, const float* mask,
                                        const float* weight, const float* bias, float* output, int B, int C,
                                        int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                                        int dh, int dw, int groups, int deformable_groups, hr_stream_t stream);
int hrnet_modulated_deform_conv_backward(const float* input, const float* offset, const float* mask,
                                         const float* weight, const float* grad_output, float* grad_input,
                                         float* grad_offset, float* grad_mask, float* grad_weight,
                                         float* grad_bias, float* scratch, int B, int C, int H, int W, int Co,
                                         int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                         int groups, int deformable_groups, hr_stream_t stream);

/*
 * K x K convolution of the Convolutional Pose Machine (nn.Conv2d of lib/models/CPM.py:11-66: 5x5, 9x9, 11x11 and 1x1
 * layers with bias, F.relu behind most of them): f32 NHWC, odd ks <= 11, stride 1, padding ks/2, implicit GEMM on the
 * f32 MFMA (csrc/conv_kxk.hip). hrnet_conv2d above serves ks 1 and 3 only.
 *   x     [N,H,W,ldx]; the Cin input channels are [x_off, x_off + Cin) of each pixel (Cin, ldx, x_off multiples of 4)
 *   w     hrnet_pack_weights mode 0 in HR_F32: [Cout rounded up to 16][ks*ks][Cin]
 *   bias  optional [Cout] f32; relu 1: y = max(y, 0)
 *   y     [N,H,W,ldy]; the Cout output channels are [y_off, y_off + Cout) of each pixel, any Cout >= 1. Nothing outside
 *         that slice is written: a producer writes its part of a concatenated map (CPM.py:91) in place.
 * dtype: HR_F32 only. The summation order is fixed and independent of N (csrc/conv_kxk.hip states it): two launches give
 * equal bits. Anything else (even ks, ks > 11, alignment, a slice outside ld) is HR_E_BADARG and writes nothing.
 */
int hrnet_conv2d_kxk(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cin,
                     int ldx, int x_off, int Cout, int ldy, int y_off, int ks, int relu, hr_stream_t stream);
/* constants of that kernel: which 0 = pixel-tile height, 1 = pixel-tile width, 2 = input channels staged per pass,
 * 3 = largest ks; anything else 0 */
hr_value_t hrnet_conv_kxk_tile(int which);
/* nn.MaxPool2d(3, 2, 1) (CPM.py:12-27) on f32 NHWC: x [N,H,W,ldx] channels [x_off, x_off + C) -> y [N,Ho,Wo,ldy] channels
 * [y_off, y_off + C), Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1; the padding never wins (-inf semantics) */
int hrnet_maxpool2d_3x3s2(const float* x, float* y, int N, int H, int W, int C, int ldx, int x_off, int ldy, int y_off,
                          hr_stream_t stream);
/* nn.AvgPool2d(9, 8, 1) of the centre map (CPM.py:10; count_include_pad: always / 81): x [N,1,H,W] f32 -> channel y_off
 * of y [N,Ho,Wo,ldy], Ho = (H-7)/8 + 1, Wo = (W-7)/8 + 1; H, W >= 7 (torch refuses a smaller map as well) */
int hrnet_avgpool2d_9s8(const float* x, float* y, int N, int H, int W, int ldy, int y_off, hr_stream_t stream);

/*
 * Training of the Convolutional Pose Machine (csrc/conv_kxk_train.hip): the backward of hrnet_conv2d_kxk and of
 * hrnet_maxpool2d_3x3s2. f32 NHWC, channel slices as above, no atomics, a fixed summation order (stated at the top of the
 * source file): two runs from the same state give equal bits. Anything an entry cannot serve is HR_E_BADARG before
 * the first launch, and nothing is written.
 *
 * conv2d_kxk_wgrad_scratch: pure host query: *bytes of scratch and *nsplit pixel-tile splits that conv2d_kxk_wgrad uses
 *   for this shape and, if split_tiles != NULL, the 8 x 16 pixel tiles of one split (the last one holds what is left).
 *   A function of the shape alone (csrc/conv_kxk_split.h).
 * conv2d_kxk_wgrad: dw[co][ci][r][s] = sum_{n,h,w} dy[n,h,w,co] x[n,h+r-p,w+s-p,ci], p = ks/2, in the Conv2d layout
 *   (Cout, Cin_real, ks, ks), overwritten; db (optional) [Cout] = sum_{n,h,w} dy.
 *   x   [N,H,W,ldx] read at channels [x_off, x_off + Cin) (Cin, ldx, x_off multiples of 4, x 16-byte aligned); only the
 *       first Cin_real <= Cin of them have a gradient (the image layers' fourth channel and the concatenated map's pad
 *       are never written). Cin == 4 runs an arrangement of its own (four taps x four channels per MFMA).
 *   dy  [N,H,W,ldy] read at channels [y_off, y_off + Cout), any Cout >= 1, any offset.
 *   scratch: the partial sums of the splits, at least *bytes of the query; a second launch adds them in split order.
 * conv2d_kxk_dgrad: dx[n,h,w,ci] = sum_{co,r,s} dy[n,h-r+p,w-s+p,co] w[co][ci][r][s] as the forward convolution of dy on
 *   the forward's own tile body:
 *   dy  [N,H,W,ldy] read at [y_off, y_off + Cout): Cout, ldy, y_off multiples of 4 (pad channels of dy hold zeros)
 *   wT  hrnet_pack_weights mode 0 of the weight permuted to (Cin, Cout, ks, ks) and flipped in both kernel axes:
 *       [Cin rounded up to 16][ks*ks][Cout]
 *   dx  [N,H,W,ldx] written at [x_off, x_off + Cin), any Cin >= 1, nothing else touched
 *   mask optional [N,H,W,ldm] read at [m_off, m_off + Cin): the result is zeroed where mask <= 0 (the ReLU of the layer
 *       that produced this input: its saved output); accumulate 1: the (masked) result is added onto what dx holds.
 * maxpool2d_3x3s2_bwd: dx[n,h,w,c] = sum of dy over the windows whose arg-max (h, w) is - the forward's rule: first
 *   maximum in (dh, dw) scan order, padding skipped, a NaN wins; relu_mask 1: times (x > 0), the backward of the ReLU
 *   that produced x. x [N,H,W,ldx] at x_off, dy [N,Ho,Wo,lddy] at dy_off, dx [N,H,W,lddx] at dx_off (overwritten).
 */
int hrnet_conv2d_kxk_wgrad_scratch(int dtype, int N, int H, int W, int Cin, int Cout, int ks, HR_HOST long long* bytes,
                                   HR_HOST int* nsplit, HR_HOST long long* split_tiles);
int hrnet_conv2d_kxk_wgrad(int dtype, const void* x, const void* dy, void* scratch, long long scratch_bytes, float* dw,
                           float* db, int N, int H, int W, int Cin, int Cin_real, int ldx, int x_off, int Cout, int ldy,
                           int y_off, int ks, hr_stream_t stream);
int hrnet_conv2d_kxk_dgrad(int dtype, const void* dy, const void* wT, void* dx, const float* mask, int N, int H, int W,
                           int Cout, int ldy, int y_off, int Cin, int ldx, int x_off, int ldm, int m_off, int ks,
                           int accumulate, hr_stream_t stream);
int hrnet_maxpool2d_3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int ldx, int x_off,
                              int lddy, int dy_off, int lddx, int dx_off, int relu_mask, hr_stream_t stream);

/*
 * The head of FTLMultiviewNet (lib/models/FTL_encoder_decoder.py; csrc/ftl.hip), f32 NHWC, inference.
 *
 * The feature transform layer reads a map per channel as 3-vectors: triplets of consecutive pixels in row-major order
 * (H W a multiple of 3; a triplet may cross a row boundary), and maps each by an affine x -> x A + c of its view.
 * coef: device [B V][12] f32, A row-major (9) then c (3), slot b V + v. Each output is
 * fma(x2, A[2][j], fma(x1, A[1][j], fma(x0, A[0][j], c[j]))) in that order.
 * ftl_gather:  x [B V,H,W,ldx] channels [x_off, x_off + C) -> y [B,H,W,ldy], view v into channels
 *   [y_off + v slice, y_off + v slice + C): the concatenation over the views is written in place. Channels of a slice past
 *   C are not written.
 * ftl_scatter: f [B,H,W,ldf] channels [f_off, f_off + C) -> y [B V,H,W,ldy] channels [y_off, y_off + C), slot b V + v, all
 *   V views from one read of f.
 * C, slice, every ld and offset are multiples of 4 and the maps 16-byte aligned; a slice outside its row, or H W no
 * multiple of 3, is HR_E_BADARG and nothing is written.
 *
 * conv2d_3x3g: a 3x3 convolution with an explicit output size, implicit GEMM on the f32 MFMA:
 *   y[n,ho,wo,co] = relu?(bias[co] + sum_{r,s,ci} w[co][3 r + s][ci] xz[n, ho stride + r - pad_lo, wo stride + s - pad_lo, ci])
 *   xz[i] = x[i / z] when i % z == 0 and 0 <= i / z < H (W), else 0
 * stride 1 or 2, pad_lo 0 .. 2, z 1 or (with stride 1) 2. Conv2d(3, stride 2, padding 2) is (2, 2, 1) with
 * Ho = (H + 1) / 2 + 1; ConvTranspose2d(3, stride 2, padding 2, output_padding op) is (1, 0, 2) with Ho = 2 H - 3 + op on the
 * flipped, transposed weight (hrnet_pack_weights mode 1); for z = 2 only the taps that meet no stuffed zero are issued.
 *   x [N,H,W,ldx] read at [x_off, x_off + Cin) (Cin, ldx, x_off multiples of 4); w [Cout rounded up to 16][9][Cin];
 *   bias optional [Cout]; y [N,Ho,Wo,ldy] written at [y_off, y_off + Cout), any Cout >= 1, nothing else touched.
 *   Ho must lie between the output size with no padding behind the (stuffed) map and that with two rows of it, Wo
 *   likewise: anything else is HR_E_BADARG. dtype: HR_F32 only. The summation order is fixed and independent of N
 *   (csrc/ftl.hip states it).
 */
int hrnet_ftl_gather(const float* x, const float* coef, float* y, int B, int V, int H, int W, int C, int ldx, int x_off,
                     int ldy, int y_off, int slice, hr_stream_t stream);
int hrnet_ftl_scatter(const float* f, const float* coef, float* y, int B, int V, int H, int W, int C, int ldf, int f_off,
                      int ldy, int y_off, hr_stream_t stream);
int hrnet_conv2d_3x3g(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cin,
                      int ldx, int x_off, int Cout, int ldy, int y_off, int Ho, int Wo, int stride, int pad_lo, int z,
                      int relu, hr_stream_t stream);

/*
 * Training of FTLMultiviewNet's head (csrc/ftl_train.hip): the backward of the two feature transforms and the weight
 * gradient of hrnet_conv2d_3x3g at z = 1. f32 NHWC, channel slices as above, no atomics, a fixed summation order (stated
 * at the top of the source file): two runs from the same state give equal bits. Anything an entry cannot serve is
 * HR_E_BADARG before the first launch, and nothing is written. The cameras carry no gradient; coef is the forward's.
 *
 * ftl_gather_bwd: dx[b V + v] = dcat[b, slice v] A_bv^T per triplet and channel:
 *   dx_i = fma(d2, A[i][2], fma(d1, A[i][1], d0 A[i][0])); the translation c plays no part.
 *   dcat [B,H,W,ldd] read at channels [d_off + v slice, d_off + v slice + C) -> dx [B V,H,W,ldx] written at
 *   [x_off, x_off + C), nothing else touched.
 * ftl_scatter_bwd: df[b] = sum_v dy[b V + v] A_bv^T, the views added in order v = 0 .. V-1 inside one thread:
 *   acc_i = 0; for v: acc_i = fma(d2, A[i][2], fma(d1, A[i][1], fma(d0, A[i][0], acc_i))).
 *   dy [B V,H,W,ldy] read at [y_off, y_off + C) -> df [B,H,W,ldf] written once at [f_off, f_off + C).
 * C, slice, every ld and offset are multiples of 4 and the maps 16-byte aligned, H W a multiple of 3, as in the forward.
 *
 * conv2d_3x3g_wgrad_scratch: pure host query: *bytes of scratch and *nsplit pixel-tile splits that conv2d_3x3g_wgrad uses
 *   for N maps of Ho x Wo outputs and, if split_tiles != NULL, the 8 x 16 output-pixel tiles of one split. A function of
 *   the shape alone (csrc/ftl_train_plan.h, on the rule of csrc/conv_kxk_split.h).
 * conv2d_3x3g_wgrad: dw[co][ci][r][s] = sum_{n,ho,wo} dy[n,ho,wo,co] x[n, ho stride + r - pad_lo, wo stride + s - pad_lo, ci]
 *   (x = 0 outside the map), stride 1 or 2, pad_lo 0 .. 2, in the Conv2d layout (Cout, Cin_real, 3, 3), overwritten.
 *   x   [N,H,W,ldx] read at [x_off, x_off + Cin) (Cin, ldx, x_off multiples of 4, x 16-byte aligned); the first
 *       Cin_real <= Cin channels have a gradient.
 *   dy  [N,Ho,Wo,ldy] read at [y_off, y_off + Cout), any Cout >= 1, any offset. Ho and Wo must lie in the size range of
 *       hrnet_conv2d_3x3g with z = 1 for H, W, stride and pad_lo.
 *   scratch: the partial sums of the splits, at least *bytes of the query; a second launch adds them in split order.
 *   The weight gradient of ConvTranspose2d(3, 2, 2, op) is this entry with the roles swapped: x := the layer's output
 *   gradient, dy := the layer's input, stride 2, pad_lo 2, Ho := the input's height; the result (Cin_T, Cout_T, 3, 3) is
 *   the ConvTranspose2d layout as it stands.
 */
int hrnet_ftl_gather_bwd(const float* dcat, const float* coef, float* dx, int B, int V, int H, int W, int C, int ldd,
                         int d_off, int slice, int ldx, int x_off, hr_stream_t stream);
int hrnet_ftl_scatter_bwd(const float* dy, const float* coef, float* df, int B, int V, int H, int W, int C, int ldy,
                          int y_off, int ldf, int f_off, hr_stream_t stream);
int hrnet_conv2d_3x3g_wgrad_scratch(int dtype, int N, int Ho, int Wo, int Cin, int Cout, HR_HOST long long* bytes,
                                    HR_HOST int* nsplit, HR_HOST long long* split_tiles);
int hrnet_conv2d_3x3g_wgrad(int dtype, const void* x, const void* dy, void* scratch, long long scratch_bytes, float* dw,
                            int N, int H, int W, int Cin, int Cin_real, int ldx, int x_off, int Cout, int ldy, int y_off,
                            int Ho, int Wo, int stride, int pad_lo, hr_stream_t stream);

/*
 * The bridge from the CPM backbone's f32 NHWC maps to the volumetric half's f32 NCHW maps (csrc/upsample_slice.hip):
 * a channel slice of an NHWC map, resampled bilinearly with align_corners, written as NCHW.
 *
 * upsample_slice_nchw: dst [N,C,H,W] = F.interpolate(src[..., c0 : c0 + C] as NCHW, size = (H, W), mode = 'bilinear',
 *   align_corners = True), src [N,h,w,Cp]. Positions as torch computes them: scale = float(in - 1) / float(out - 1) (0 when
 *   out == 1), pos = scale * index in f32, lower = int(pos), upper = lower + (lower < in - 1), lambda = pos - lower; the
 *   value is (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11). Any h, w, H, W >= 1 (down-sampling and equal
 *   sizes included), any 0 <= c0, C >= 1, c0 + C <= Cp; no alignment beyond that of a float.
 * upsample_slice_nchw_bwd: the exact transpose in gather form: every element of the slice of dsrc [N,h,w,Cp] is the sum,
 *   Y ascending then X ascending, of weight(Y, y) weight(X, x) ddst[n][c][Y][X] over its footprint (the outputs that name
 *   it as a neighbour, found from the same f32 positions). One thread owns one element: no atomics, equal bits on every
 *   run. accumulate 0 writes the slice (zero where nothing reads a source pixel), 1 adds onto what is there; channels
 *   outside [c0, c0 + C) keep their bits in both modes.
 * upsample_slice_nchw_supported: 1 when [c0, c0 + C) is a slice of a row of Cp channels, else 0.
 * Anything an entry cannot serve (a null or aliased pointer, an empty axis, a map of 2^31 pixels, a slice outside its
 * row) is HR_E_BADARG before the launch, and nothing is written.
 */
int hrnet_upsample_slice_nchw(const float* src, float* dst, int N, int h, int w, int Cp, int c0, int C,
                              int H, int W, hr_stream_t stream);
int hrnet_upsample_slice_nchw_bwd(const float* ddst, float* dsrc, int N, int h, int w, int Cp, int c0, int C,
                                  int H, int W, int accumulate, hr_stream_t stream);
hr_value_t hrnet_upsample_slice_nchw_supported(int Cp, int c0, int C);

/*
 * The spatio-temporal LSTM cell of PredRNN between its convolutions (lib/models/predrnn.py:33-58 of the reference) and
 * the MaxPool2d(2, 2) of the model's ResNet tail (csrc/predrnn.hip). f32 NHWC, inference, no atomics, a fixed summation
 * order (stated at the top of the source file): two runs give equal bits. Anything an entry cannot serve is HR_E_BADARG
 * before the first launch, and nothing is written. Every map is 16-byte aligned.
 *
 * sample_stats: nn.LayerNorm([C, W, W])'s statistics: for up to three dense maps x_m [B, n_m] (n_m = H W C_m elements per
 *   sample, a multiple of 4; n_m = 0 and x_m = NULL: map absent, the maps present first) stats[(m B + b) 2] = mean and
 *   [.. + 1] = rstd = 1 / sqrt(var + eps) of sample b of map m, var the biased variance. All sums in double on data shifted
 *   by the sample's first element, rounded to float once. scratch: at least *bytes of sample_stats_scratch (a pure host
 *   query, a function of the shape alone: csrc/predrnn_plan.h), 8-byte aligned.
 * stlstm_gates: xc [B,H,W,7 nh] (slices i f g i' f' g' o), hc [B,H,W,4 nh] (i f g o), mc [B,H,W,3 nh] (i f g): the raw
 *   outputs of conv_x, conv_h, conv_m; stats [3][B][2] of sample_stats over them in that order; wx, bx [H,W,7 nh], wh, bh
 *   [H,W,4 nh], wm, bm [H,W,3 nh]: the LayerNorm weights and biases repacked from (C, H, W). With
 *   LN(v) = fma((v - mean) rstd, w, b):
 *     c_new = sigmoid(i_x + i_h) tanh(g_x + g_h) + sigmoid(f_x + f_h + 1) c_t     -> mem channels [0, nh)
 *     m_new = sigmoid(i'_x + i_m) tanh(g'_x + g_m) + sigmoid(f'_x + f_m + 1) m_t  -> mem channels [nh, 2 nh)
 *     o_pre = o_x + o_h                                                           -> o_pre [B,H,W,nh]
 *   c_t [B,H,W,ldc] read at [c_off, c_off + nh), m_t [B,H,W,ldmt] at [m_off, m_off + nh), mem [B,H,W,ldmem], nothing outside
 *   its first 2 nh channels written; nh, every ld and offset multiples of 4. c_t may be mem's own slice [0, nh) and m_t its
 *   slice [nh, 2 nh) (same pointer and row length): every thread reads its own elements before it writes them. Any other
 *   overlap of an input with an output is refused.
 * stlstm_out: h_new [B,H,W,nh] = sigmoid(o_pre + LN(oc)) tanh(last): oc the raw conv_o output with its stats [B][2] and
 *   affine wo, bo [H,W,nh]; last the conv_last output.
 * maxpool2d_2x2: nn.MaxPool2d(2, 2): x [N,H,W,ldx] channels [x_off, x_off + C) -> y [N,H/2,W/2,ldy] channels
 *   [y_off, y_off + C); even H and W; C, every ld and offset multiples of 4; a NaN wins.
 */
int hrnet_sample_stats_scratch(int B, long long n0, long long n1, long long n2, HR_HOST long long* bytes);
int hrnet_sample_stats(const float* x0, const float* x1, const float* x2, long long n0, long long n1, long long n2, int B,
                       double eps, void* scratch, long long scratch_bytes, float* stats, hr_stream_t stream);
int hrnet_stlstm_gates(const float* xc, const float* hc, const float* mc, const float* stats, const float* wx,
                       const float* bx, const float* wh, const float* bh, const float* wm, const float* bm,
                       const float* c_t, int ldc, int c_off, const float* m_t, int ldmt, int m_off, float* mem, int ldmem,
                       float* o_pre, int B, int H, int W, int nh, hr_stream_t stream);
int hrnet_stlstm_out(const float* oc, const float* stats, const float* wo, const float* bo, const float* o_pre,
                     const float* last, float* h_new, int B, int H, int W, int nh, hr_stream_t stream);
int hrnet_maxpool2d_2x2(const float* x, float* y, int N, int H, int W, int C, int ldx, int x_off, int ldy, int y_off,
                        hr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HRNET_HIP_H */
