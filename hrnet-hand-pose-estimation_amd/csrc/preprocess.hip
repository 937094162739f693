// Input step of tools/inference.py: a ragged batch of u8 HWC images (any size, all in one device buffer) ->
// bilinear resize to the model's input size (cv2 INTER_LINEAR geometry: half-pixel centres, edge clamp, no
// antialiasing) -> the ToTensor + Normalize of normalize_u8_kernel (loss.hip), NCHW f32. One launch per batch.
//
// Per output slot s (blockIdx.y) the slot table gives {byte offset, H, W, row pitch}; several slots may name the
// same source bytes (the PoseAggr frame windows). A row that does not fit the buffer is never read: its whole
// output plane becomes NaN, the other slots are unaffected.
//
// Geometry: sx = (x + 0.5) * W / Wo - 0.5 = ((2x + 1) W - Wo) / (2 Wo). The numerator and denominator are integers,
// so x0 = floor(sx) is an exact integer division and fx = remainder / (2 Wo) is one correctly rounded f32 division
// (exact operands while 2 Wo < 2^24): no f32 error in the source position. At 1920 -> 256 the f32 product
// (x + 0.5f) * 7.5f - 0.5f is off by up to 1.2e-4 px, which moves the blended value by up to 0.03 of a u8 code.
// Identity size gives fx = 0 exactly, an exact 2x downscale fx = 0.5 exactly.
#include "common.h"

namespace {

// source index and weight of output coordinate o along an axis of n source / m output pixels (cv2 INTER_LINEAR:
// a negative position clamps to pixel 0 with weight 0; i1 = min(i0 + 1, n - 1))
__device__ __forceinline__ void rn_axis(int o, int n, int m, int& i0, int& i1, float& f) {
  const long long num = (2LL * o + 1) * n - m, den = 2LL * m;
  if (num <= 0) {
    i0 = 0;
    f = 0.f;
  } else {
    const unsigned long long q = (unsigned long long)num / (unsigned long long)den;
    i0 = (int)q;
    f = (float)(num - (long long)q * den) / (float)den;
  }
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
}

__global__ __launch_bounds__(256) void resize_normalize_u8_kernel(const unsigned char* __restrict__ src,
                                                                  long long src_bytes,
                                                                  const long long* __restrict__ slots,
                                                                  float* __restrict__ out, int Ho, int Wo, float m0,
                                                                  float m1, float m2, float s0, float s1, float s2,
                                                                  int bgr) {
  const int s = blockIdx.y;
  const long long hw = (long long)Ho * Wo;
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;      // hw <= 2^30 (host check)
  if (p >= hw) return;
  float* o = out + (long long)s * 3 * hw + p;
  // wave-uniform row: scalar loads
  const long long off = slots[4LL * s], H = slots[4LL * s + 1], W = slots[4LL * s + 2], pitch = slots[4LL * s + 3];
  // every term is checked before it is multiplied, so that a corrupt row cannot overflow the extent test
  const bool ok = off >= 0 && off <= src_bytes && H > 0 && W > 0 && H <= 0x7fffffff && W <= 0x7fffffff &&
                  W <= (src_bytes - off) / 3 && pitch >= 3 * W &&
                  (H - 1) <= (src_bytes - off - 3 * W) / pitch;
  if (!ok) {
    const float nan = __builtin_nanf("");
    o[0] = nan;
    o[hw] = nan;
    o[2 * hw] = nan;
    return;
  }
  const int y = p / Wo, x = p - y * Wo;
  int x0, x1, y0, y1;
  float fx, fy;
  rn_axis(x, (int)W, Wo, x0, x1, fx);
  rn_axis(y, (int)H, Ho, y0, y1, fy);
  // 64-bit addresses: offsets may exceed 2^31 (bounded by the extent test above)
  const unsigned char* r0 = src + off + (long long)y0 * pitch;
  const unsigned char* r1 = src + off + (long long)y1 * pitch;
  const long long c0 = 3LL * x0, c1 = 3LL * x1;
  const float gx = 1.f - fx, gy = 1.f - fy;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ch = bgr ? 2 - c : c;
    const float a = (float)r0[c0 + ch], b = (float)r0[c1 + ch];
    const float d = (float)r1[c0 + ch], e = (float)r1[c1 + ch];
    const float v = gy * (gx * a + fx * b) + fy * (gx * d + fx * e);
    // cv2 saturate_cast<uchar>: round half to even, clamp
    const float u = fminf(fmaxf(__builtin_rintf(v), 0.f), 255.f);
    // the expression of normalize_u8_kernel: bit-identical to it at Ho == H, Wo == W
    o[c * hw] = (u / 255.f - mean[c]) / sd[c];
  }
}

}  // namespace

extern "C" int hrnet_resize_normalize_u8(const unsigned char* src, int64_t src_bytes, const int64_t* slots, int n,
                                         float* out_nchw, int Ho, int Wo, const float* mean3, const float* std3,
                                         int bgr, hr_stream_t stream) {
  HR_REQUIRE(src && slots && out_nchw && mean3 && std3 && src_bytes > 0, "resize_normalize_u8: null argument");
  HR_REQUIRE(n > 0 && n <= 65535, "resize_normalize_u8: n = %d slots (1..65535)", n);
  HR_REQUIRE(Ho > 0 && Wo > 0 && (long long)Ho * Wo <= (1LL << 30), "resize_normalize_u8: output %d x %d", Ho, Wo);
  HR_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "resize_normalize_u8: zero std");
  const long long hw = (long long)Ho * Wo;
  const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(resize_normalize_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, (long long)src_bytes,
                     (const long long*)slots, out_nchw, Ho, Wo, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                     std3[2], bgr);
  return hr_check_launch("resize_normalize_u8");
}

// ---------------------------------------------------------------------------------------------------------------------
// Training input step of the RHD reader (lib/dataset/rhd.py; reference lib/dataset/transforms/transforms.py:74-175):
// the crop -> cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) to Ho x Wo -> optional horizontal flip -> ToTensor +
// Normalize, for a whole batch in one launch. The slot table is the one above; a crop is a slot that points into its
// image (offset of the crop's top-left byte, crop H and W, the image's row pitch), so the bytes around the crop are
// never read: they count as 0 like everything else outside the slot.
//
// Per output pixel (x, y): (sx, sy) = M (x, y, 1) with M the slot's 2x3 INVERSE matrix (output pixel -> crop pixel,
// the flip folded in by the host). The position is formed in f64 from the f32 matrix entries: in f32 a coordinate
// near 300 px is off by up to 3e-5 px, which at a 0 -> 255 edge moves the blend by 8e-3 of a u8 code. Bilinear blend
// of the four neighbours floor(sx) + {0,1} x floor(sy) + {0,1} in f32; a neighbour outside [0,W) x [0,H) contributes
// 0. The blend is rounded half to even and clamped to a u8 code, then normalised with the expression of
// normalize_u8_kernel, so an identity matrix at Ho == H, Wo == W is bit-identical to hrnet_normalize_u8.
// cv2 instead quantises the position to 1/32 px and the weights to 15 bits; that deviation is documented, not pinned.
namespace {

__global__ __launch_bounds__(256) void affine_warp_normalize_u8_kernel(const unsigned char* __restrict__ src,
                                                                       long long src_bytes,
                                                                       const long long* __restrict__ slots,
                                                                       const float* __restrict__ inv,
                                                                       float* __restrict__ out, int Ho, int Wo,
                                                                       float m0, float m1, float m2, float s0,
                                                                       float s1, float s2) {
  const int s = blockIdx.y;
  const long long hw = (long long)Ho * Wo;
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;      // hw <= 2^30 (host check)
  if (p >= hw) return;
  float* o = out + (long long)s * 3 * hw + p;
  const long long off = slots[4LL * s], H = slots[4LL * s + 1], W = slots[4LL * s + 2], pitch = slots[4LL * s + 3];
  // the row checks of resize_normalize_u8_kernel: a row outside the buffer is never read, its plane is NaN
  const bool ok = off >= 0 && off <= src_bytes && H > 0 && W > 0 && H <= 0x7fffffff && W <= 0x7fffffff &&
                  W <= (src_bytes - off) / 3 && pitch >= 3 * W &&
                  (H - 1) <= (src_bytes - off - 3 * W) / pitch;
  if (!ok) {
    const float nan = __builtin_nanf("");
    o[0] = nan;
    o[hw] = nan;
    o[2 * hw] = nan;
    return;
  }
  const int y = p / Wo, x = p - y * Wo;
  const float* m = inv + 6LL * s;
  const double sx = (double)m[0] * x + (double)m[1] * y + (double)m[2];
  const double sy = (double)m[3] * x + (double)m[4] * y + (double)m[5];
  const double fx0 = floor(sx), fy0 = floor(sy);
  float v[3] = {0.f, 0.f, 0.f};
  // some neighbour lies inside only when floor(s) is in [-1, W-1]; false for NaN too (a non-finite matrix gives 0)
  if (fx0 >= -1.0 && fx0 <= (double)(W - 1) && fy0 >= -1.0 && fy0 <= (double)(H - 1)) {
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
    const float gx = 1.f - fx, gy = 1.f - fy;
    // clamped indices keep every read inside the slot; a neighbour outside it is masked to 0 below
    const bool in_x0 = x0 >= 0, in_x1 = x0 + 1 < W, in_y0 = y0 >= 0, in_y1 = y0 + 1 < H;
    const long long xa = in_x0 ? x0 : 0, xb = in_x1 ? x0 + 1 : W - 1;
    const long long ya = in_y0 ? y0 : 0, yb = in_y1 ? y0 + 1 : H - 1;
    const unsigned char* r0 = src + off + ya * pitch;
    const unsigned char* r1 = src + off + yb * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = (in_y0 && in_x0) ? (float)r0[3 * xa + c] : 0.f;
      const float b = (in_y0 && in_x1) ? (float)r0[3 * xb + c] : 0.f;
      const float d = (in_y1 && in_x0) ? (float)r1[3 * xa + c] : 0.f;
      const float e = (in_y1 && in_x1) ? (float)r1[3 * xb + c] : 0.f;
      v[c] = gy * (gx * a + fx * b) + fy * (gx * d + fx * e);
    }
  }
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = fminf(fmaxf(__builtin_rintf(v[c]), 0.f), 255.f);
    o[c * hw] = (u / 255.f - mean[c]) / sd[c];
  }
}

}  // namespace

extern "C" int hrnet_affine_warp_normalize_u8(const unsigned char* src, int64_t src_bytes, const int64_t* slots,
                                              const float* inv_mats, int n, float* out_nchw, int Ho, int Wo,
                                              const float* mean3, const float* std3, hr_stream_t stream) {
  HR_REQUIRE(src && slots && inv_mats && out_nchw && mean3 && std3 && src_bytes > 0,
             "affine_warp_normalize_u8: null argument");
  HR_REQUIRE(n > 0 && n <= 65535, "affine_warp_normalize_u8: n = %d slots (1..65535)", n);
  HR_REQUIRE(Ho > 0 && Wo > 0 && (long long)Ho * Wo <= (1LL << 30), "affine_warp_normalize_u8: output %d x %d", Ho,
             Wo);
  HR_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "affine_warp_normalize_u8: zero std");
  const long long hw = (long long)Ho * Wo;
  const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(affine_warp_normalize_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, src,
                     (long long)src_bytes, (const long long*)slots, inv_mats, out_nchw, Ho, Wo, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2]);
  return hr_check_launch("affine_warp_normalize_u8");
}
