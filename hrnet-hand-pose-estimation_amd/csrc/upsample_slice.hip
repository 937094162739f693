// The bridge between the f32 NHWC maps of the CPM backbone and the f32 NCHW maps of the volumetric half
// (include/hrnet_hip.h: hrnet_upsample_slice_nchw, hrnet_upsample_slice_nchw_bwd):
//
//   dst[n][c][Y][X] = bilinear, align_corners, of src[n][.][.][c0 + c]      src [N,h,w,Cp] NHWC, dst [N,C,H,W] NCHW
//
// A layout change with four reads per output, so memory bound; both sides are touched along their fast axis:
//
//   forward   one workgroup = US_PIX consecutive output pixels (Y W + X, flattened, so a narrow map still fills the
//             lanes) x US_CH channels of one image. Lanes run along the CHANNELS while they read the four neighbours
//             of a pixel (runs of C floats in an NHWC row) and blend; the blended value goes to LDS transposed,
//             tile[c][pixel] with a row of US_PIX + 1 floats, so the 32 lanes of a store group (one pixel, channels
//             c .. c + 31) hit the banks (c + pixel) mod 32, all different. Then lanes run along the PIXELS, read LDS
//             rows consecutively and store US_PIX consecutive floats of one channel plane.
//   backward  the mirror: one workgroup = US_PIX consecutive SOURCE pixels x US_CH channels. Lanes run along the
//             pixels while each thread gathers its footprint from one plane of ddst (neighbouring lanes read
//             neighbouring runs of a row of W), sums it in a register in the fixed order Y ascending, X ascending,
//             stores tile[c][pixel], and then lanes run along the channels to write (or add onto) the slice of the
//             NHWC row. No atomics: one thread owns one source element, so two runs give equal bits.
//
// The tile is a run of flattened pixels, not a rectangle, so LDS use does not depend on any of h, w, H, W, C.
//
// Positions are torch's (aten UpSampleBilinear2d, align_corners): scale = float(in - 1) / float(out - 1) (0 when
// out == 1), pos = scale * index rounded to f32, lower = int(pos), upper = lower + (lower < in - 1), lambda = pos - lower.
// The value is (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11). The footprint of a source row y is
// the output rows whose lower neighbour is y - 1 or y, found by bisection on the SAME f32 position, so the backward
// is the exact transpose of the forward, roundings of the position included.
#include "common.h"

#define US_PIX 64
#define US_CH 32
#define US_LD (US_PIX + 1)
#define US_THREADS 256
#define US_PER ((US_PIX * US_CH) / US_THREADS)

struct UsArgs {
  int N, h, w, Cp, c0, C, H, W;
  float sy, sx;          // (h - 1) / (H - 1), (w - 1) / (W - 1)
  long long tiles;       // pixel tiles per image
  int chunks;            // channel chunks
};

// lower neighbour of output index i (clamped so that no rounding can step outside the map)
__device__ __forceinline__ int us_lower(float scale, int i, int in, float* pos) {
  const float p = __fmul_rn(scale, (float)i);
  int l = (int)p;
  l = l > in - 1 ? in - 1 : l;
  *pos = p;
  return l;
}

// first index in [0, out) whose lower neighbour is >= v (out if none): the lower neighbour is monotone in the index
__device__ __forceinline__ int us_first(float scale, int in, int out, int v) {
  int lo = 0, hi = out;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    float p;
    if (us_lower(scale, mid, in, &p) >= v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// weight of source index s in output index i: (lower == s) (1 - lambda) + (upper == s) lambda
__device__ __forceinline__ float us_weight(float scale, int i, int in, int s) {
  float p;
  const int l = us_lower(scale, i, in, &p);
  const int u = l + (l < in - 1 ? 1 : 0);
  const float lam = p - (float)l;
  return (l == s ? 1.0f - lam : 0.0f) + (u == s ? lam : 0.0f);
}

__global__ __launch_bounds__(US_THREADS) void us_fwd_kernel(const float* __restrict__ src, float* __restrict__ dst, UsArgs a) {
  __shared__ float tile[US_CH * US_LD];
  __shared__ int s_o[4][US_PIX];
  __shared__ float s_l[2][US_PIX];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int chunk = (int)(b % a.chunks);
  const long long t = b / a.chunks;
  const long long ti = t % a.tiles;
  const int n = (int)(t / a.tiles);
  const long long HW = (long long)a.H * a.W;
  if (tid < US_PIX) {
    const long long P = ti * US_PIX + tid;
    if (P < HW) {
      const int Y = (int)(P / a.W), X = (int)(P % a.W);
      float py, px;
      const int y0 = us_lower(a.sy, Y, a.h, &py), x0 = us_lower(a.sx, X, a.w, &px);
      const int y1 = y0 + (y0 < a.h - 1 ? 1 : 0), x1 = x0 + (x0 < a.w - 1 ? 1 : 0);
      s_o[0][tid] = y0 * a.w + x0; s_o[1][tid] = y0 * a.w + x1;
      s_o[2][tid] = y1 * a.w + x0; s_o[3][tid] = y1 * a.w + x1;
      s_l[0][tid] = py - (float)y0; s_l[1][tid] = px - (float)x0;
    } else {
      s_o[0][tid] = -1;
    }
  }
  __syncthreads();
  const float* base = src + (size_t)n * a.h * a.w * a.Cp + a.c0 + chunk * US_CH;
#pragma unroll
  for (int i = 0; i < US_PER; ++i) {
    const int idx = tid + US_THREADS * i;
    const int c = idx & (US_CH - 1), p = idx / US_CH;
    const int o00 = s_o[0][p];
    if (o00 >= 0 && chunk * US_CH + c < a.C) {
      const float ly = s_l[0][p], lx = s_l[1][p];
      const float v00 = base[(size_t)o00 * a.Cp + c], v01 = base[(size_t)s_o[1][p] * a.Cp + c];
      const float v10 = base[(size_t)s_o[2][p] * a.Cp + c], v11 = base[(size_t)s_o[3][p] * a.Cp + c];
      const float hx = 1.0f - lx, hy = 1.0f - ly;
      tile[c * US_LD + p] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < US_PER; ++i) {
    const int idx = tid + US_THREADS * i;
    const int p = idx & (US_PIX - 1), c = idx / US_PIX;
    const long long P = ti * US_PIX + p;
    const int cc = chunk * US_CH + c;
    if (P < HW && cc < a.C) dst[((size_t)n * a.C + cc) * HW + P] = tile[c * US_LD + p];
  }
}

__global__ __launch_bounds__(US_THREADS) void us_bwd_kernel(const float* __restrict__ ddst, float* __restrict__ dsrc, UsArgs a,
                                                            int accumulate) {
  __shared__ float tile[US_CH * US_LD];
  __shared__ int s_r[4][US_PIX];     // Y first, Y end, X first, X end of the pixel's footprint
  __shared__ int s_q[2][US_PIX];     // the source pixel's y and x
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int chunk = (int)(b % a.chunks);
  const long long t = b / a.chunks;
  const long long ti = t % a.tiles;
  const int n = (int)(t / a.tiles);
  const long long hw = (long long)a.h * a.w, HW = (long long)a.H * a.W;
  if (tid < US_PIX) {
    const long long q = ti * US_PIX + tid;
    if (q < hw) {
      const int y = (int)(q / a.w), x = (int)(q % a.w);
      s_q[0][tid] = y; s_q[1][tid] = x;
      s_r[0][tid] = us_first(a.sy, a.h, a.H, y - 1); s_r[1][tid] = us_first(a.sy, a.h, a.H, y + 1);
      s_r[2][tid] = us_first(a.sx, a.w, a.W, x - 1); s_r[3][tid] = us_first(a.sx, a.w, a.W, x + 1);
    } else {
      s_q[0][tid] = -1;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < US_PER; ++i) {
    const int idx = tid + US_THREADS * i;
    const int p = idx & (US_PIX - 1), c = idx / US_PIX;
    const int cc = chunk * US_CH + c;
    const int y = s_q[0][p];
    if (y >= 0 && cc < a.C) {
      const int x = s_q[1][p];
      const int Ya = s_r[0][p], Yb = s_r[1][p], Xa = s_r[2][p], Xb = s_r[3][p];
      const float* g = ddst + ((size_t)n * a.C + cc) * HW;
      float acc = 0.0f;
      for (int Y = Ya; Y < Yb; ++Y) {
        const float wy = us_weight(a.sy, Y, a.h, y);
        const float* row = g + (size_t)Y * a.W;
        for (int X = Xa; X < Xb; ++X) acc = fmaf(wy * us_weight(a.sx, X, a.w, x), row[X], acc);
      }
      tile[c * US_LD + p] = acc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < US_PER; ++i) {
    const int idx = tid + US_THREADS * i;
    const int c = idx & (US_CH - 1), p = idx / US_CH;
    const long long q = ti * US_PIX + p;
    const int cc = chunk * US_CH + c;
    if (q < hw && cc < a.C) {
      float* o = dsrc + ((size_t)n * hw + q) * a.Cp + a.c0 + cc;
      const float v = tile[c * US_LD + p];
      *o = accumulate ? *o + v : v;
    }
  }
}

extern "C" hr_value_t hrnet_upsample_slice_nchw_supported(int Cp, int c0, int C) {
  return (c0 >= 0 && C >= 1 && (long long)c0 + C <= Cp) ? 1 : 0;
}

// checks shared by both directions; `pix` is the pixel count of the side the workgroups tile
static int us_args(const char* what, const void* a0, const void* a1, int N, int h, int w, int Cp, int c0, int C, int H, int W,
                   long long pix, UsArgs* a, long long* blocks) {
  HR_REQUIRE(a0 && a1 && a0 != a1, "%s: null or aliased argument", what);
  HR_REQUIRE((((uintptr_t)a0 | (uintptr_t)a1) & 3) == 0, "%s: pointers must be 4-byte aligned", what);
  HR_REQUIRE(N >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "%s: N = %d, h = %d, w = %d, H = %d, W = %d", what, N, h, w, H, W);
  HR_REQUIRE(hrnet_upsample_slice_nchw_supported(Cp, c0, C), "%s: channels [%d, %d + %d) do not lie in a row of %d", what, c0,
             c0, C, Cp);
  const long long lim = 2147483647LL - US_PIX;
  HR_REQUIRE((long long)h * w <= lim && (long long)H * W <= lim, "%s: a map of %d x %d or %d x %d has too many pixels", what,
             h, w, H, W);
  a->N = N; a->h = h; a->w = w; a->Cp = Cp; a->c0 = c0; a->C = C; a->H = H; a->W = W;
  a->sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f;
  a->sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
  a->tiles = (pix + US_PIX - 1) / US_PIX;
  a->chunks = (C + US_CH - 1) / US_CH;
  HR_REQUIRE(a->tiles <= 2147483647LL / a->chunks / N, "%s: N = %d, %lld pixel tiles, %d channel chunks: too many workgroups",
             what, N, a->tiles, a->chunks);
  *blocks = a->tiles * a->chunks * N;
  return 0;
}

extern "C" int hrnet_upsample_slice_nchw(const float* src, float* dst, int N, int h, int w, int Cp, int c0, int C, int H, int W,
                                         hr_stream_t stream) {
  UsArgs a;
  long long blocks;
  const int rc = us_args("upsample_slice_nchw", src, dst, N, h, w, Cp, c0, C, H, W, (long long)H * W, &a, &blocks);
  if (rc) return rc;
  hipLaunchKernelGGL(us_fwd_kernel, dim3((unsigned)blocks), dim3(US_THREADS), 0, (hipStream_t)stream, src, dst, a);
  return hr_check_launch("upsample_slice_nchw");
}

extern "C" int hrnet_upsample_slice_nchw_bwd(const float* ddst, float* dsrc, int N, int h, int w, int Cp, int c0, int C, int H,
                                             int W, int accumulate, hr_stream_t stream) {
  UsArgs a;
  long long blocks;
  HR_REQUIRE(accumulate == 0 || accumulate == 1, "upsample_slice_nchw_bwd: accumulate = %d", accumulate);
  const int rc = us_args("upsample_slice_nchw_bwd", ddst, dsrc, N, h, w, Cp, c0, C, H, W, (long long)h * w, &a, &blocks);
  if (rc) return rc;
  hipLaunchKernelGGL(us_bwd_kernel, dim3((unsigned)blocks), dim3(US_THREADS), 0, (hipStream_t)stream, ddst, dsrc, a, accumulate);
  return hr_check_launch("upsample_slice_nchw_bwd");
}
