// Training of the Convolutional Pose Machine: weight gradient and data gradient of the K x K convolution of
// csrc/conv_kxk.hip (odd ks <= 11, stride 1, padding ks/2) and the backward of MaxPool2d(3, 2, 1). f32 NHWC, channel
// slices (ld, off, C) on every map, only real channels stored, no atomics.
//
// hrnet_conv2d_kxk_wgrad: dW[co][ci][r][s] = sum_{n,h,w} dy[n,h,w,co] x[n,h+r-p,w+s-p,ci] on v_mfma_f32_16x16x4_f32 with
// FOUR NEIGHBOURING PIXELS OF ONE ROW as the K of an MFMA: A = dy (16 output channels x 4 pixels), B = the input window
// shifted by the tap (4 pixels x 16 input channels), D = one tap's 16 x 16 block of dW. A workgroup of four waves owns
// one 16 x 16 block for all ks*ks taps, tap u on wave u % 4 (at most 31 accumulators of four registers per wave), and
// walks a range of 8 x 16 pixel tiles: per tile the dy tile and the (8 + ks - 1) x (16 + ks - 1) input window of the 16
// input channels are staged in LDS ONCE and every tap reads its shifted B operand from there (no im2col in global
// memory). The pixel tiles are split over workgroups (csrc/conv_kxk_split.h states the rule: a function of the shape
// alone); the partial blocks go to scratch and a second launch adds them IN SPLIT ORDER and writes the Conv2d layout
// (Cout, Cin_real, ks, ks): padded input channels and rows >= Cout are never written.
//
// Summation order of one dW[co][ci][r][s] (fixed; two runs give equal bits):
//   for split k = 0 .. nsplit-1:  part_k = 0
//     for tile t = k per .. min((k+1) per, tiles) - 1   (n-major, then tile row, then tile column)
//       for h = 0 .. 7 (rows of the tile inside the map); for w4 = 0, 4, 8, 12 (inside the map):
//         part_k = mfma_16x16x4(dy[h][w4 + g][co], x[h + r - p][w4 + g + s - p][ci], g = 0 .. 3, part_k)
//     (a pixel outside the map contributes dy = 0, a window position outside it x = 0)
//   dW = ((part_0 + part_1) + part_2) + ...
// The bias gradient db[co] = sum dy rides along: the workgroups of input-channel block 0 run one more MFMA per pixel
// group against B = 1 (every column of its D is the pixel sum of dy), so db has the same order: per split the chain over
// tiles and pixel groups, then the splits in order.
// Cin == 4 (the image layers, 3 real channels): the 16 columns of D are FOUR NEIGHBOURING TAPS of a kernel row x 4
// channels, column 4 j + c = tap (r, s0 + j), channel c, so a 9 x 9 kernel is 9 x 3 units instead of 81 quarter-used
// ones. The LDS window is [pixel][4], and the B operand of the unit (r, s0) is again 64 consecutive floats.
// Columns of taps past the row end are computed on whatever follows in LDS and dropped by the reduce pass.
//
// hrnet_conv2d_kxk_dgrad: dx = conv(dy, flipped transposed weight) on the tile body of the forward (conv_kxk_body.h: its
// summation order is that of hrnet_conv2d_kxk with dy for x), epilogue: zero where mask <= 0 (NaN mask: zero), then add
// the destination if accumulate.
//
// hrnet_maxpool2d_3x3s2_bwd: gather form, one thread per input element: for the at most four windows that hold it, in
// (ho, wo) order, the window's arg-max is recomputed by the forward's rule (first maximum in (dh, dw) scan order,
// padding skipped, a NaN wins) and dy is added where the element is it; optionally times (x > 0).
#include "conv_kxk_body.h"
#include "conv_kxk_split.h"

namespace {

static_assert(KXW_TH == KX_TH && KXW_TW == KX_TW && KXW_MAXKS == KX_MAXKS, "the plan header and the tile body agree");

struct KxwArgs {
  const float* x;
  const float* dy;
  float* scratch;
  int N, H, W, Cin, ldx, x_off, Cout, ldy, y_off, tiles_h, tiles_w, cit;
  long long tiles, per, split_floats, bias_at;
};

template <int KS, bool CIN4>
__global__ __launch_bounds__(256) void kxk_wgrad_kernel(const KxwArgs a) {
  constexpr int SG = (KS + 3) / 4;
  constexpr int UNITS = CIN4 ? KS * SG : KS * KS;
  constexpr int UPW = (UNITS + 3) / 4;
  constexpr int CH = CIN4 ? 4 : 16;
  constexpr int PAD = KS / 2, HH = KX_TH + KS - 1, WH = KX_TW + KS - 1;
  constexpr int XW = (HH * WH + 8) * CH;   // + 8 pixels: what a four-tap group past the row end reads (Cin == 4)
  extern __shared__ float kw_lds[];
  float* xw = kw_lds;
  float* dyt = kw_lds + XW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int cot_i = (int)blockIdx.x / a.cit, cit_i = (int)blockIdx.x % a.cit;
  const int co0 = cot_i * 16, ci0 = cit_i * 16;
  const int k = blockIdx.y;
  const bool do_bias = wave == 3 && cit_i == 0;

  int off[UPW];
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    const int u = wave + 4 * j;
    const int r = CIN4 ? u / SG : u / KS, s = CIN4 ? (u % SG) * 4 : u % KS;
    off[j] = u < UNITS ? (r * WH + s) * CH : 0;   // a unit past the last one recomputes unit 0 and is dropped
  }
  f32x4 acc[UPW], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < UPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long t_end = (k + 1) * a.per < a.tiles ? (k + 1) * a.per : a.tiles;
  for (long long t = k * a.per; t < t_end; ++t) {
    const int tw = (int)(t % a.tiles_w);
    const long long t2 = t / a.tiles_w;
    const int th = (int)(t2 % a.tiles_h), n = (int)(t2 / a.tiles_h);
    const int h0 = th * KX_TH, w0 = tw * KX_TW;
    const float* xn = a.x + (size_t)n * a.H * a.W * a.ldx + a.x_off;
    const float* dyn = a.dy + (size_t)n * a.H * a.W * a.ldy + a.y_off;
    __syncthreads();   // the MFMAs of the previous tile have read both buffers
    if constexpr (CIN4) {
      for (int p = tid; p < HH * WH; p += 256) {
        const int hr = p / WH, wc = p - hr * WH;
        const int h = h0 + hr - PAD, w = w0 + wc - PAD;
        V16 v = v16_zero();
        if (h >= 0 && h < a.H && w >= 0 && w < a.W) v = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx);
        *(V16*)(xw + p * 4) = v;
      }
      if (tid < 8) *(V16*)(xw + (HH * WH + tid) * 4) = v16_zero();
    } else {
      for (int v = tid; v < HH * WH * 4; v += 256) {
        const int p = v >> 2, g = v & 3;
        const int hr = p / WH, wc = p - hr * WH;
        const int h = h0 + hr - PAD, w = w0 + wc - PAD, c = ci0 + g * 4;
        V16 val = v16_zero();
        if (h >= 0 && h < a.H && w >= 0 && w < a.W && c < a.Cin) val = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx + c);
        *(V16*)(xw + v * 4) = val;
      }
    }
    for (int v = tid; v < KX_TH * KX_TW * 16; v += 256) {
      const int p = v >> 4, c = v & 15;
      const int h = h0 + (p >> 4), w = w0 + (p & 15), co = co0 + c;
      dyt[v] = h < a.H && w < a.W && co < a.Cout ? dyn[((size_t)h * a.W + w) * a.ldy + co] : 0.f;
    }
    __syncthreads();
    const int rows = a.H - h0 < KX_TH ? a.H - h0 : KX_TH;
    const int wq_n = a.W - w0 < KX_TW ? (a.W - w0 + 3) >> 2 : KX_TW / 4;
    for (int h = 0; h < rows; ++h)
      for (int wq = 0; wq < wq_n; ++wq) {
        const float av = dyt[(h * KX_TW + wq * 4 + lg) * 16 + li];
        const float* xb = xw + (h * WH + wq * 4 + lg) * CH + li;
#pragma unroll
        for (int j = 0; j < UPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[off[j]], acc[j], 0, 0, 0);
        if (do_bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
      }
  }

  // D: column = lane & 15, row (output channel) = 4 (lane >> 4) + register; a block of scratch is [unit][16 co][16 col]
  float* sp = a.scratch + (size_t)k * a.split_floats;
  float* blk = sp + (size_t)blockIdx.x * UNITS * 256;
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    const int u = wave + 4 * j;
    if (u >= UNITS) continue;
    const float o[4] = {acc[j].x, acc[j].y, acc[j].z, acc[j].w};
#pragma unroll
    for (int q = 0; q < 4; ++q) blk[(size_t)u * 256 + (lg * 4 + q) * 16 + li] = o[q];
  }
  if (do_bias && li == 0) {
    const float o[4] = {accb.x, accb.y, accb.z, accb.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) sp[a.bias_at + co0 + lg * 4 + q] = o[q];
  }
}

// dw[co][ci][r][s] and db[co]: the splits' partials added in split order
__global__ __launch_bounds__(256) void kxk_wgrad_reduce_kernel(const float* __restrict__ scratch, float* __restrict__ dw,
                                                               float* __restrict__ db, int nsplit, long long split_floats,
                                                               long long bias_at, int Cout, int Cin_real, int ks, int cit,
                                                               int cin4, long long total_w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int taps = ks * ks, sg = (ks + 3) >> 2;
  long long idx;
  float* dst;
  if (e < total_w) {
    const int tap = (int)(e % taps);
    const long long e2 = e / taps;
    const int ci = (int)(e2 % Cin_real), co = (int)(e2 / Cin_real);
    if (cin4) {
      const int r = tap / ks, s = tap - r * ks;
      idx = ((long long)(co >> 4) * (ks * sg) + r * sg + (s >> 2)) * 256 + (co & 15) * 16 + (s & 3) * 4 + ci;
    } else {
      idx = (((long long)(co >> 4) * cit + (ci >> 4)) * taps + tap) * 256 + (co & 15) * 16 + (ci & 15);
    }
    dst = dw + e;
  } else if (db && e < total_w + Cout) {
    idx = bias_at + (e - total_w);
    dst = db + (e - total_w);
  } else {
    return;
  }
  float sum = scratch[idx];
  for (int k = 1; k < nsplit; ++k) sum += scratch[(size_t)k * split_floats + idx];
  *dst = sum;
}

template <int KS>
void kxw_launch(const KxwArgs& a, int cin4, unsigned blocks, unsigned nsplit, hipStream_t s) {
  constexpr int HH = KX_TH + KS - 1, WH = KX_TW + KS - 1;
  const dim3 grid(blocks, nsplit);
  if (cin4)
    hipLaunchKernelGGL((kxk_wgrad_kernel<KS, true>), grid, dim3(256), (size_t)((HH * WH + 8) * 4 + KX_TH * KX_TW * 16) * 4, s,
                       a);
  else
    hipLaunchKernelGGL((kxk_wgrad_kernel<KS, false>), grid, dim3(256), (size_t)((HH * WH + 8) * 16 + KX_TH * KX_TW * 16) * 4,
                       s, a);
}

// MaxPool2d(3, 2, 1) backward, gather form: one thread per (input pixel, channel)
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ dx, int N, int H, int W, int C, int ldx,
                                                               int x_off, int lddy, int dy_off, int lddx, int dx_off, int Ho,
                                                               int Wo, int relu_mask) {
  const long long total = (long long)N * H * W * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long long p = i / C;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H), n = (int)(p / H);
    const float* xn = x + (size_t)n * H * W * ldx + x_off + c;
    float g = 0.f;
    // the windows that hold (h, w): ho with |h - 2 ho| <= 1
    for (int ho = h >> 1; ho <= (h + 1) >> 1 && ho < Ho; ++ho)
      for (int wo = w >> 1; wo <= (w + 1) >> 1 && wo < Wo; ++wo) {
        float m = -INFINITY;
        int ah = -1, aw = -1;
        for (int dh = -1; dh <= 1; ++dh) {
          const int hh = 2 * ho + dh;
          if (hh < 0 || hh >= H) continue;
          for (int dw = -1; dw <= 1; ++dw) {
            const int ww = 2 * wo + dw;
            if (ww < 0 || ww >= W) continue;
            const float v = xn[((size_t)hh * W + ww) * ldx];
            if (ah < 0 || v > m || v != v) {   // the forward's rule; a window of -inf alone keeps its first element
              m = v;
              ah = hh;
              aw = ww;
            }
          }
        }
        if (ah == h && aw == w) g += dy[(((size_t)n * Ho + ho) * Wo + wo) * lddy + dy_off + c];
      }
    if (relu_mask && !(xn[((size_t)h * W + w) * ldx] > 0.f)) g = 0.f;
    dx[(((size_t)n * H + h) * W + w) * lddx + dx_off + c] = g;
  }
}

unsigned kxt_ew_grid(long long total) {
  const long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

int kxw_check(const char* who, int dtype, int N, int H, int W, int Cin, int Cout, int ks, KxwPlan* p) {
  HR_REQUIRE(dtype == HR_F32, "%s: dtype = %d: only f32 (HR_F32 = 0) is built", who, dtype);
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "%s: N = %d, H = %d, W = %d, Cin = %d, Cout = %d", who, N, H, W,
             Cin, Cout);
  HR_REQUIRE(ks >= 1 && ks <= KX_MAXKS && (ks & 1), "%s: ks = %d (odd, 1 .. %d)", who, ks, KX_MAXKS);
  HR_REQUIRE(Cin % 4 == 0, "%s: Cin = %d: a multiple of 4 (the slice read, padding included)", who, Cin);
  HR_REQUIRE(kxw_plan(N, H, W, Cin, Cout, ks, p), "%s: N = %d, H = %d, W = %d, Cin = %d, Cout = %d: more pixel tiles or "
             "channel blocks than 2^31 - 1", who, N, H, W, Cin, Cout);
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_conv2d_kxk_wgrad_scratch(int dtype, int N, int H, int W, int Cin, int Cout, int ks, long long* bytes,
                                              int* nsplit, long long* split_tiles) {
  HR_REQUIRE(bytes && nsplit, "conv2d_kxk_wgrad_scratch: null argument");
  KxwPlan p;
  const int rc = kxw_check("conv2d_kxk_wgrad_scratch", dtype, N, H, W, Cin, Cout, ks, &p);
  if (rc != HR_OK) return rc;
  *bytes = p.bytes;
  *nsplit = p.nsplit;
  if (split_tiles) *split_tiles = p.per;
  return HR_OK;
}

extern "C" int hrnet_conv2d_kxk_wgrad(int dtype, const void* x, const void* dy, void* scratch, long long scratch_bytes,
                                      float* dw, float* db, int N, int H, int W, int Cin, int Cin_real, int ldx, int x_off,
                                      int Cout, int ldy, int y_off, int ks, hr_stream_t stream) {
  KxwPlan p;
  const int rc = kxw_check("conv2d_kxk_wgrad", dtype, N, H, W, Cin, Cout, ks, &p);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(x && dy && scratch && dw, "conv2d_kxk_wgrad: null argument");
  HR_REQUIRE(Cin_real >= 1 && Cin_real <= Cin, "conv2d_kxk_wgrad: %d real of Cin = %d", Cin_real, Cin);
  HR_REQUIRE(ldx % 4 == 0 && x_off % 4 == 0 && ((uintptr_t)x & 15) == 0,
             "conv2d_kxk_wgrad: ldx = %d, x_off = %d: multiples of 4, x 16-byte aligned", ldx, x_off);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + Cin <= ldx, "conv2d_kxk_wgrad: channels [%d, %d + %d) outside ldx = %d", x_off,
             x_off, Cin, ldx);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + Cout <= ldy, "conv2d_kxk_wgrad: channels [%d, %d + %d) outside ldy = %d", y_off,
             y_off, Cout, ldy);
  HR_REQUIRE((((uintptr_t)dy | (uintptr_t)scratch | (uintptr_t)dw | (uintptr_t)db) & 3) == 0,
             "conv2d_kxk_wgrad: dy, scratch, dw and db must be 4-byte aligned");
  HR_REQUIRE(scratch_bytes >= p.bytes, "conv2d_kxk_wgrad: scratch of %lld bytes, %lld needed (hrnet_conv2d_kxk_wgrad_scratch)",
             scratch_bytes, p.bytes);
  const long long total_w = (long long)Cout * Cin_real * ks * ks;
  const long long rblocks = (total_w + Cout + 255) / 256;
  HR_REQUIRE(rblocks <= 0x7fffffffLL, "conv2d_kxk_wgrad: %lld weight gradients", total_w);
  KxwArgs a;
  a.x = (const float*)x; a.dy = (const float*)dy; a.scratch = (float*)scratch;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.x_off = x_off; a.Cout = Cout; a.ldy = ldy; a.y_off = y_off;
  a.tiles_h = p.tiles_h; a.tiles_w = p.tiles_w; a.cit = p.cit; a.tiles = p.tiles; a.per = p.per;
  a.split_floats = p.split_floats; a.bias_at = p.blocks * p.units * 256;
  const hipStream_t s = (hipStream_t)stream;
  switch (ks) {
    case 1: kxw_launch<1>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
    case 3: kxw_launch<3>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
    case 5: kxw_launch<5>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
    case 7: kxw_launch<7>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
    case 9: kxw_launch<9>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
    default: kxw_launch<11>(a, p.cin4, (unsigned)p.blocks, (unsigned)p.nsplit, s); break;
  }
  hipLaunchKernelGGL(kxk_wgrad_reduce_kernel, dim3((unsigned)rblocks), dim3(256), 0, s, (const float*)scratch, dw, db, p.nsplit,
                     p.split_floats, a.bias_at, Cout, Cin_real, ks, p.cit, p.cin4, total_w);
  return hr_check_launch("conv2d_kxk_wgrad");
}

extern "C" int hrnet_conv2d_kxk_dgrad(int dtype, const void* dy, const void* wT, void* dx, const float* mask, int N, int H,
                                      int W, int Cout, int ldy, int y_off, int Cin, int ldx, int x_off, int ldm, int m_off,
                                      int ks, int accumulate, hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "conv2d_kxk_dgrad: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(dy && wT && dx, "conv2d_kxk_dgrad: null argument");
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "conv2d_kxk_dgrad: N = %d, H = %d, W = %d, Cin = %d, Cout = %d",
             N, H, W, Cin, Cout);
  HR_REQUIRE(ks >= 1 && ks <= KX_MAXKS && (ks & 1), "conv2d_kxk_dgrad: ks = %d (odd, 1 .. %d)", ks, KX_MAXKS);
  HR_REQUIRE(Cout % 4 == 0 && ldy % 4 == 0 && y_off % 4 == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)wT & 15) == 0,
             "conv2d_kxk_dgrad: Cout = %d, ldy = %d, y_off = %d: multiples of 4 (zero pad channels in dy), dy and wT 16-byte "
             "aligned", Cout, ldy, y_off);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + Cout <= ldy, "conv2d_kxk_dgrad: channels [%d, %d + %d) outside ldy = %d", y_off,
             y_off, Cout, ldy);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + Cin <= ldx, "conv2d_kxk_dgrad: channels [%d, %d + %d) outside ldx = %d", x_off,
             x_off, Cin, ldx);
  HR_REQUIRE(!mask || (m_off >= 0 && (long long)m_off + Cin <= ldm), "conv2d_kxk_dgrad: mask channels [%d, %d + %d) outside ldm = %d",
             m_off, m_off, Cin, ldm);
  HR_REQUIRE(((uintptr_t)dx & 3) == 0 && ((uintptr_t)mask & 3) == 0 && (accumulate == 0 || accumulate == 1),
             "conv2d_kxk_dgrad: dx / mask alignment, accumulate = %d", accumulate);
  HR_REQUIRE(dx != dy && (const void*)mask != (const void*)dy, "conv2d_kxk_dgrad: dy is aliased by dx or mask");
  KxkArgs a;
  a.x = (const float*)dy; a.w = (const float*)wT; a.bias = nullptr; a.y = (float*)dx;
  a.N = N; a.H = H; a.W = W; a.Cin = Cout; a.ldx = ldy; a.x_off = y_off; a.Cout = Cin;
  a.ldy = ldx; a.y_off = x_off; a.ks = ks; a.relu = 0;
  a.vec_store = ldx % 4 == 0 && x_off % 4 == 0 && ((uintptr_t)dx & 15) == 0;
  a.mask = mask; a.ldm = ldm; a.m_off = m_off; a.accumulate = accumulate;
  return kx_dispatch<true>(a, "conv2d_kxk_dgrad", (hipStream_t)stream);
}

extern "C" int hrnet_maxpool2d_3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int ldx,
                                         int x_off, int lddy, int dy_off, int lddx, int dx_off, int relu_mask,
                                         hr_stream_t stream) {
  HR_REQUIRE(x && dy && dx, "maxpool2d_3x3s2_bwd: null argument");
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, "maxpool2d_3x3s2_bwd: N = %d, H = %d, W = %d, C = %d", N, H, W, C);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + C <= ldx && dy_off >= 0 && (long long)dy_off + C <= lddy && dx_off >= 0 &&
                 (long long)dx_off + C <= lddx,
             "maxpool2d_3x3s2_bwd: channels [%d, +%d) in ldx = %d, [%d, +%d) in lddy = %d, [%d, +%d) in lddx = %d", x_off, C, ldx,
             dy_off, C, lddy, dx_off, C, lddx);
  HR_REQUIRE(dx != x && dx != dy, "maxpool2d_3x3s2_bwd: dx is aliased by x or dy");
  HR_REQUIRE(relu_mask == 0 || relu_mask == 1, "maxpool2d_3x3s2_bwd: relu_mask = %d", relu_mask);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(kxt_ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, x,
                     dy, dx, N, H, W, C, ldx, x_off, lddy, dy_off, lddx, dx_off, Ho, Wo, relu_mask);
  return hr_check_launch("maxpool2d_3x3s2_bwd");
}
