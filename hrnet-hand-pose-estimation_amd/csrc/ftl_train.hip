// Training of FTLMultiviewNet's head: the backward of the two feature transforms of csrc/ftl.hip and the weight gradient
// of its general 3x3 convolution (hrnet_conv2d_3x3g at z = 1: stride 1 or 2, pad_lo 0 .. 2, explicit output size). f32
// NHWC, channel slices (ld, off, C) on every map, no atomics.
//
// hrnet_ftl_gather_bwd / hrnet_ftl_scatter_bwd. The forward maps a triplet x (three consecutive pixels of one channel) to
// y = x A + c, so the gradient of a triplet is d A^T and the translation plays no part. One thread takes a triplet x 4
// channels as the forward does: three 16-byte loads per view, 3 x 4 outputs, three 16-byte stores, the grid rule of the
// forward (one thread per work item in 256-thread blocks, a grid-stride loop beyond 2048 blocks).
//   gather_bwd:  dx_i = fma(d2, A[i][2], fma(d1, A[i][1], d0 A[i][0])),  d = channel slice v of the concatenated map's
//                gradient, one view per thread.
//   scatter_bwd: acc_i = 0; for v = 0 .. V-1: acc_i = fma(d2, A[i][2], fma(d1, A[i][1], fma(d0, A[i][0], acc_i)));
//                df_i = acc_i: the views are added in order inside one thread, every dy is read once and df written once.
//
// hrnet_conv2d_3x3g_wgrad: dW[co][ci][r][s] = sum_{n,ho,wo} dy[n,ho,wo,co] x[n, ho S + r - pad_lo, wo S + s - pad_lo, ci]
// on v_mfma_f32_16x16x4_f32 in the arrangement of kxk_wgrad_kernel (csrc/conv_kxk_train.hip): FOUR NEIGHBOURING OUTPUT
// PIXELS OF ONE ROW are the K of an MFMA, A = dy (16 output channels x 4 pixels), B = the input window at the tap's
// offset and at pixel stride S (4 pixels x 16 input channels), D = one tap's 16 x 16 block of dW. A workgroup of four
// waves owns one 16 x 16 block for all nine taps (tap u on wave u % 4: three accumulators per wave) and walks a range of
// 8 x 16 output-pixel tiles; per tile the dy tile and the (7 S + 3) x (15 S + 3) input window of the 16 input channels are
// staged in LDS once. The tiles are split over workgroups by the plan of csrc/ftl_train_plan.h (a function of the shape
// alone); the partial blocks go to scratch and a second launch adds them IN SPLIT ORDER and writes the Conv2d layout
// (Cout, Cin_real, 3, 3): padded input channels and rows >= Cout are never written.
//
// LDS banks of the B operand (read from the code below; ds_read_b32: bank = dword address mod 32, the two 32-lane halves
// of a wave are served separately). A lane reads dword ((row S + r) WH + col(w, s)) 16 + ci with ci = lane & 15 and
// w = 4 wq + (lane >> 4). With the window stored in column order, col = w S + s, a 32-lane half reads pixels w and w + 1:
// at S = 1 dwords [0, 16) and [16, 32) of one 32-dword row - all 32 banks once; at S = 2 dwords [0, 16) and [32, 48) - the
// same 16 banks twice, a 2-way conflict on every B read of the inner loop. So at S = 2 the window's columns are stored
// DE-INTERLEAVED: the even columns of a row first (17 of the 33), then the odd ones, col = (s & 1) 17 + (s >> 1) + w. A
// tap reads columns of one parity only, its four pixels are again neighbours in LDS, and the half-wave reads 32
// consecutive dwords as at S = 1: conflict-free. The A operand (dy tile [pixel][16]) reads 64 consecutive dwords either
// way. The staging stores are 16-byte (ds_write_b128) of four consecutive lanes per pixel; de-interleaving moves whole
// 64-byte pixels and leaves their pattern as it is.
//
// Summation order of one dW[co][ci][r][s] (fixed; two runs give equal bits):
//   for split k = 0 .. nsplit-1:  part_k = 0
//     for tile t = k per .. min((k+1) per, tiles) - 1   (n-major, then tile row, then tile column, of the Ho x Wo map)
//       for h = 0 .. 7 (rows of the tile inside the map); for w4 = 0, 4, 8, 12 (inside the map):
//         part_k = mfma_16x16x4(dy[h][w4 + g][co], x[h S + r - pad_lo][(w4 + g) S + s - pad_lo][ci], g = 0 .. 3, part_k)
//     (an output pixel outside the map contributes dy = 0, a window position outside the input x = 0)
//   dW = ((part_0 + part_1) + part_2) + ...
#include "conv_kxk_body.h"
#include "ftl_train_plan.h"

namespace {

static_assert(KXW_TH == KX_TH && KXW_TW == KX_TW, "the plan header and the tile body agree");

struct G3wArgs {
  const float* x;
  const float* dy;
  float* scratch;
  int N, H, W, Cin, ldx, x_off, Cout, ldy, y_off, Ho, Wo, pad_lo, tiles_h, tiles_w, cit;
  long long tiles, per, split_floats;
};

template <int S>
__global__ __launch_bounds__(256) void g3w_kernel(const G3wArgs a) {
  constexpr int HH = (KX_TH - 1) * S + 3, WH = (KX_TW - 1) * S + 3;
  constexpr int WHE = (WH + 1) / 2;        // even columns of a window row (S = 2)
  constexpr int XW = HH * WH * 16;
  extern __shared__ float gw_lds[];
  float* xw = gw_lds;
  float* dyt = gw_lds + XW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int cot_i = (int)blockIdx.x / a.cit, cit_i = (int)blockIdx.x % a.cit;
  const int co0 = cot_i * 16, ci0 = cit_i * 16;
  const int k = blockIdx.y;

  // tap u = wave + 4 j; where its B operand starts in the window. A unit past the ninth recomputes tap 0 and is dropped
  int off[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int u = wave + 4 * j;
    const int r = u / 3, s = u % 3;
    const int col = S == 2 ? (s & 1) * WHE + (s >> 1) : s;
    off[j] = u < 9 ? (r * WH + col) * 16 : 0;
  }
  f32x4 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long t_end = (k + 1) * a.per < a.tiles ? (k + 1) * a.per : a.tiles;
  for (long long t = k * a.per; t < t_end; ++t) {
    const int tw = (int)(t % a.tiles_w);
    const long long t2 = t / a.tiles_w;
    const int th = (int)(t2 % a.tiles_h), n = (int)(t2 / a.tiles_h);
    const int h0 = th * KX_TH, w0 = tw * KX_TW;
    const int h_first = h0 * S - a.pad_lo, w_first = w0 * S - a.pad_lo;
    const float* xn = a.x + (size_t)n * a.H * a.W * a.ldx + a.x_off;
    const float* dyn = a.dy + (size_t)n * a.Ho * a.Wo * a.ldy + a.y_off;
    __syncthreads();   // the MFMAs of the previous tile have read both buffers
    for (int v = tid; v < HH * WH * 4; v += 256) {
      const int p = v >> 2, g = v & 3;
      const int hr = p / WH, wc = p - hr * WH;
      const int h = h_first + hr, w = w_first + wc, c = ci0 + g * 4;
      V16 val = v16_zero();
      if (h >= 0 && h < a.H && w >= 0 && w < a.W && c < a.Cin) val = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx + c);
      const int col = S == 2 ? (wc & 1) * WHE + (wc >> 1) : wc;
      *(V16*)(xw + ((hr * WH + col) * 4 + g) * 4) = val;
    }
    for (int v = tid; v < KX_TH * KX_TW * 16; v += 256) {
      const int p = v >> 4, c = v & 15;
      const int h = h0 + (p >> 4), w = w0 + (p & 15), co = co0 + c;
      dyt[v] = h < a.Ho && w < a.Wo && co < a.Cout ? dyn[((size_t)h * a.Wo + w) * a.ldy + co] : 0.f;
    }
    __syncthreads();
    const int rows = a.Ho - h0 < KX_TH ? a.Ho - h0 : KX_TH;
    const int wq_n = a.Wo - w0 < KX_TW ? (a.Wo - w0 + 3) >> 2 : KX_TW / 4;
    for (int h = 0; h < rows; ++h)
      for (int wq = 0; wq < wq_n; ++wq) {
        const float av = dyt[(h * KX_TW + wq * 4 + lg) * 16 + li];
        const float* xb = xw + (h * S * WH + wq * 4 + lg) * 16 + li;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[off[j]], acc[j], 0, 0, 0);
      }
  }

  // D: column (input channel) = lane & 15, row (output channel) = 4 (lane >> 4) + register; a block of scratch is
  // [tap][16 co][16 ci]
  float* blk = a.scratch + (size_t)k * a.split_floats + (size_t)blockIdx.x * 9 * 256;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int u = wave + 4 * j;
    if (u >= 9) continue;
    const float o[4] = {acc[j].x, acc[j].y, acc[j].z, acc[j].w};
#pragma unroll
    for (int q = 0; q < 4; ++q) blk[(size_t)u * 256 + (lg * 4 + q) * 16 + li] = o[q];
  }
}

// dw[co][ci][r][s]: the splits' partials added in split order
__global__ __launch_bounds__(256) void g3w_reduce_kernel(const float* __restrict__ scratch, float* __restrict__ dw, int nsplit,
                                                         long long split_floats, int Cin_real, int cit, long long total_w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total_w) return;
  const int tap = (int)(e % 9);
  const long long e2 = e / 9;
  const int ci = (int)(e2 % Cin_real), co = (int)(e2 / Cin_real);
  const long long idx = (((long long)(co >> 4) * cit + (ci >> 4)) * 9 + tap) * 256 + (co & 15) * 16 + (ci & 15);
  float sum = scratch[idx];
  for (int k = 1; k < nsplit; ++k) sum += scratch[(size_t)k * split_floats + idx];
  dw[e] = sum;
}

// dx (B V, P, ldx) <- slice v of dcat (B, P, ldd) times A_bv^T, per triplet of pixels and channel
__global__ __launch_bounds__(256) void ftl_gather_bwd_kernel(const float* __restrict__ dcat, const float* __restrict__ coef,
                                                             float* __restrict__ dx, int B, int V, int T, int C4, int ldd,
                                                             int d_off, int slice, int ldx, int x_off) {
  const long long total = (long long)B * V * T * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    long long q = i / C4;
    const int tr = (int)(q % T);
    const int bv = (int)(q / T), b = bv / V, v = bv - b * V;
    const float* k = coef + (size_t)bv * 12;
    const float* dp = dcat + ((size_t)b * T * 3 + (size_t)tr * 3) * ldd + d_off + (size_t)v * slice + cg * 4;
    const f32x4 d0 = *(const f32x4*)dp, d1 = *(const f32x4*)(dp + ldd), d2 = *(const f32x4*)(dp + 2 * (size_t)ldd);
    float* xp = dx + ((size_t)bv * T * 3 + (size_t)tr * 3) * ldx + x_off + cg * 4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf(d2[e], k[3 * r + 2], fmaf(d1[e], k[3 * r + 1], d0[e] * k[3 * r]));
      *(f32x4*)(xp + (size_t)r * ldx) = o;
    }
  }
}

// df (B, P, ldf) <- sum over v, in order, of dy (B V, P, ldy) slot b V + v times A_bv^T
__global__ __launch_bounds__(256) void ftl_scatter_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ coef,
                                                              float* __restrict__ df, int B, int V, int T, int C4, int ldy,
                                                              int y_off, int ldf, int f_off) {
  const long long total = (long long)B * T * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    long long q = i / C4;
    const int tr = (int)(q % T), b = (int)(q / T);
    f32x4 acc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < V; ++v) {
      const int bv = b * V + v;
      const float* k = coef + (size_t)bv * 12;
      const float* dp = dy + ((size_t)bv * T * 3 + (size_t)tr * 3) * ldy + y_off + cg * 4;
      const f32x4 d0 = *(const f32x4*)dp, d1 = *(const f32x4*)(dp + ldy), d2 = *(const f32x4*)(dp + 2 * (size_t)ldy);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[r][e] = fmaf(d2[e], k[3 * r + 2], fmaf(d1[e], k[3 * r + 1], fmaf(d0[e], k[3 * r], acc[r][e])));
    }
    float* fp = df + ((size_t)b * T * 3 + (size_t)tr * 3) * ldf + f_off + cg * 4;
#pragma unroll
    for (int r = 0; r < 3; ++r) *(f32x4*)(fp + (size_t)r * ldf) = acc[r];
  }
}

// the grid rule and the argument checks of the forward transforms (csrc/ftl.hip: ftl_grid, ftl_check)
unsigned ftlb_grid(long long total) {
  const long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int ftlb_check(const char* who, const void* src, const void* coef, const void* dst, int B, int V, int H, int W, int C,
               int ld_in, int in_off, long long in_width, int ld_out, int out_off) {
  HR_REQUIRE(src && coef && dst, "%s: null argument", who);
  HR_REQUIRE(B >= 1 && V >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: B = %d, V = %d, H = %d, W = %d, C = %d", who, B, V, H, W,
             C);
  HR_REQUIRE((long long)B * V <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL, "%s: B V = %lld, H W = %lld", who,
             (long long)B * V, (long long)H * W);
  HR_REQUIRE(((long long)H * W) % 3 == 0, "%s: H W = %d x %d = %lld pixels are no whole number of triplets", who, H, W,
             (long long)H * W);
  HR_REQUIRE(C % 4 == 0 && ld_in % 4 == 0 && in_off % 4 == 0 && ld_out % 4 == 0 && out_off % 4 == 0,
             "%s: C = %d, ld = %d / %d, offsets %d / %d: multiples of 4", who, C, ld_in, ld_out, in_off, out_off);
  HR_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)coef & 3) == 0,
             "%s: the maps must be 16-byte aligned", who);
  HR_REQUIRE(in_off >= 0 && (long long)in_off + in_width <= ld_in, "%s: input channels [%d, %d + %lld) outside ld = %d", who,
             in_off, in_off, in_width, ld_in);
  HR_REQUIRE(out_off >= 0 && (long long)out_off + C <= ld_out, "%s: output channels [%d, %d + %d) outside ld = %d", who,
             out_off, out_off, C, ld_out);
  HR_REQUIRE(src != dst, "%s: the gradient is aliased by its destination", who);
  return HR_OK;
}

int g3w_check(const char* who, int dtype, int N, int Ho, int Wo, int Cin, int Cout, KxwPlan* p) {
  HR_REQUIRE(dtype == HR_F32, "%s: dtype = %d: only f32 (HR_F32 = 0) is built", who, dtype);
  HR_REQUIRE(N >= 1 && Ho >= 1 && Wo >= 1 && Cin >= 1 && Cout >= 1, "%s: N = %d, Ho = %d, Wo = %d, Cin = %d, Cout = %d", who, N,
             Ho, Wo, Cin, Cout);
  HR_REQUIRE(Cin % 4 == 0, "%s: Cin = %d: a multiple of 4 (the slice read, padding included)", who, Cin);
  HR_REQUIRE(g3w_plan(N, Ho, Wo, Cin, Cout, p), "%s: N = %d, Ho = %d, Wo = %d, Cin = %d, Cout = %d: more pixel tiles or "
             "channel blocks than 2^31 - 1", who, N, Ho, Wo, Cin, Cout);
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_ftl_gather_bwd(const float* dcat, const float* coef, float* dx, int B, int V, int H, int W, int C,
                                    int ldd, int d_off, int slice, int ldx, int x_off, hr_stream_t stream) {
  HR_REQUIRE(slice >= C && slice % 4 == 0, "ftl_gather_bwd: slice = %d: a multiple of 4 that holds C = %d", slice, C);
  const int rc = ftlb_check("ftl_gather_bwd", dcat, coef, dx, B, V, H, W, C, ldd, d_off, (long long)(V - 1) * slice + C, ldx,
                            x_off);
  if (rc != HR_OK) return rc;
  const int T = (int)((long long)H * W / 3);
  hipLaunchKernelGGL(ftl_gather_bwd_kernel, dim3(ftlb_grid((long long)B * V * T * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     dcat, coef, dx, B, V, T, C / 4, ldd, d_off, slice, ldx, x_off);
  return hr_check_launch("ftl_gather_bwd");
}

extern "C" int hrnet_ftl_scatter_bwd(const float* dy, const float* coef, float* df, int B, int V, int H, int W, int C,
                                     int ldy, int y_off, int ldf, int f_off, hr_stream_t stream) {
  const int rc = ftlb_check("ftl_scatter_bwd", dy, coef, df, B, V, H, W, C, ldy, y_off, C, ldf, f_off);
  if (rc != HR_OK) return rc;
  const int T = (int)((long long)H * W / 3);
  hipLaunchKernelGGL(ftl_scatter_bwd_kernel, dim3(ftlb_grid((long long)B * T * (C / 4))), dim3(256), 0, (hipStream_t)stream, dy,
                     coef, df, B, V, T, C / 4, ldy, y_off, ldf, f_off);
  return hr_check_launch("ftl_scatter_bwd");
}

extern "C" int hrnet_conv2d_3x3g_wgrad_scratch(int dtype, int N, int Ho, int Wo, int Cin, int Cout, long long* bytes,
                                               int* nsplit, long long* split_tiles) {
  HR_REQUIRE(bytes && nsplit, "conv2d_3x3g_wgrad_scratch: null argument");
  KxwPlan p;
  const int rc = g3w_check("conv2d_3x3g_wgrad_scratch", dtype, N, Ho, Wo, Cin, Cout, &p);
  if (rc != HR_OK) return rc;
  *bytes = p.bytes;
  *nsplit = p.nsplit;
  if (split_tiles) *split_tiles = p.per;
  return HR_OK;
}

extern "C" int hrnet_conv2d_3x3g_wgrad(int dtype, const void* x, const void* dy, void* scratch, long long scratch_bytes,
                                       float* dw, int N, int H, int W, int Cin, int Cin_real, int ldx, int x_off, int Cout,
                                       int ldy, int y_off, int Ho, int Wo, int stride, int pad_lo, hr_stream_t stream) {
  KxwPlan p;
  const int rc = g3w_check("conv2d_3x3g_wgrad", dtype, N, Ho, Wo, Cin, Cout, &p);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(x && dy && scratch && dw, "conv2d_3x3g_wgrad: null argument");
  HR_REQUIRE(H >= 1 && W >= 1 && H <= 0x3fffffff && W <= 0x3fffffff, "conv2d_3x3g_wgrad: H = %d, W = %d", H, W);
  HR_REQUIRE((stride == 1 || stride == 2) && pad_lo >= 0 && pad_lo <= 2,
             "conv2d_3x3g_wgrad: stride = %d (1, 2), pad_lo = %d (0 .. 2)", stride, pad_lo);
  {
    long long hlo, hhi, wlo, whi;
    g3w_size_range(H, stride, pad_lo, &hlo, &hhi);
    g3w_size_range(W, stride, pad_lo, &wlo, &whi);
    HR_REQUIRE(Ho >= hlo && Ho <= hhi && Wo >= wlo && Wo <= whi,
               "conv2d_3x3g_wgrad: Ho x Wo = %d x %d: H = %d, W = %d, stride = %d, pad_lo = %d give %lld .. %lld x %lld .. %lld",
               Ho, Wo, H, W, stride, pad_lo, hlo, hhi, wlo, whi);
  }
  HR_REQUIRE(Cin_real >= 1 && Cin_real <= Cin, "conv2d_3x3g_wgrad: %d real of Cin = %d", Cin_real, Cin);
  HR_REQUIRE(ldx % 4 == 0 && x_off % 4 == 0 && ((uintptr_t)x & 15) == 0,
             "conv2d_3x3g_wgrad: ldx = %d, x_off = %d: multiples of 4, x 16-byte aligned", ldx, x_off);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + Cin <= ldx, "conv2d_3x3g_wgrad: channels [%d, %d + %d) outside ldx = %d", x_off,
             x_off, Cin, ldx);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + Cout <= ldy, "conv2d_3x3g_wgrad: channels [%d, %d + %d) outside ldy = %d", y_off,
             y_off, Cout, ldy);
  HR_REQUIRE((((uintptr_t)dy | (uintptr_t)scratch | (uintptr_t)dw) & 3) == 0,
             "conv2d_3x3g_wgrad: dy, scratch and dw must be 4-byte aligned");
  HR_REQUIRE(scratch_bytes >= p.bytes, "conv2d_3x3g_wgrad: scratch of %lld bytes, %lld needed (hrnet_conv2d_3x3g_wgrad_scratch)",
             scratch_bytes, p.bytes);
  const long long total_w = (long long)Cout * Cin_real * 9;
  const long long rblocks = (total_w + 255) / 256;
  HR_REQUIRE(rblocks <= 0x7fffffffLL, "conv2d_3x3g_wgrad: %lld weight gradients", total_w);
  G3wArgs a;
  a.x = (const float*)x; a.dy = (const float*)dy; a.scratch = (float*)scratch;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.x_off = x_off; a.Cout = Cout; a.ldy = ldy; a.y_off = y_off;
  a.Ho = Ho; a.Wo = Wo; a.pad_lo = pad_lo;
  a.tiles_h = p.tiles_h; a.tiles_w = p.tiles_w; a.cit = p.cit; a.tiles = p.tiles; a.per = p.per;
  a.split_floats = p.split_floats;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)p.nsplit);
  if (stride == 1)
    hipLaunchKernelGGL((g3w_kernel<1>), grid, dim3(256), (size_t)((KX_TH + 2) * (KX_TW + 2) * 16 + KX_TH * KX_TW * 16) * 4, s, a);
  else
    hipLaunchKernelGGL((g3w_kernel<2>), grid, dim3(256),
                       (size_t)((2 * KX_TH + 1) * (2 * KX_TW + 1) * 16 + KX_TH * KX_TW * 16) * 4, s, a);
  hipLaunchKernelGGL(g3w_reduce_kernel, dim3((unsigned)rblocks), dim3(256), 0, s, (const float*)scratch, dw, p.nsplit,
                     p.split_floats, Cin_real, p.cit, total_w);
  return hr_check_launch("conv2d_3x3g_wgrad");
}
