// Volumetric lifting (reference lib/models/triangulation_model_utils/op.py:84-168, lib/core/loss.py:225-256): the
// unprojection of every view's feature maps into a world-space voxel grid with its aggregation over the views, the 3-D
// soft-argmax over the voxel grid, and the volumetric cross-entropy term - forward and backward. All tensors f32:
// features [B,V,C,H,W], volumes [B,C,X,Y,Z], coordinate volumes [B,X,Y,Z,3], projections [B,V,3,4]. Element offsets
// are 64-bit throughout (B C X Y Z passes 2^31 bytes at a moderate batch).
//
// Sample position of voxel p in view v (vol_position, shared by the forward and the backward so that both see the same
// cell and the same weights): q = P [p, 1] in f64; the view is invalid where q.z <= 0; q.z == 0 is replaced by 1;
// u = q.x / q.z, w = q.y / q.z; column u (W - 1) / H and row w (H - 1) / W - the reference's normalisation 2 (u / H -
// 0.5), 2 (w / W - 0.5) with (H, W) = heatmap_shape fed to grid_sample(align_corners=True), swapped divisors and all; it
// is the reference's rule, not a pixel-exact one. The split into integer cell and fractional weights is f64, the blend
// of the four corners f32, a corner outside the map contributes 0 (zero padding), an invalid view samples 0.
//
// unproject_fwd_kernel: one thread per voxel, lanes along z (coalesced volume stores, neighbouring sample positions);
// a thread computes its V positions once and walks a chunk of channels. The maps are read through L1/L2 (the 2 MB of a
// sample's maps stay in L2).
//
// unproject_bwd_kernel: the input gradient is a scatter. A workgroup owns (b, v, a few channels): it keeps one plane
// per channel in LDS in 64-bit fixed point, walks the voxels of the sample, recomputes positions and samples, and adds
// each corner's share with integer LDS atomics - integer addition commutes, so the plane is the same bits on every run
// (the scheme of csrc/dcn.hip) - then stores the planes with plain stores. The fixed-point scale of a plane comes from
// bounds the workgroup computes itself before the walk: max |gV[b, c]| times the largest per-view factor of the
// method (1; |conf|; 1 + 2 max |features[b, :, c]| for softmax).
//
// volume_integrate: a map has X Y Z voxels and there are only B J maps, so a map is split over kVolSplit workgroups:
// partials (max, sum, three moments) per workgroup, every workgroup of the second launch merges its map's partials in
// index order and normalises its own chunk. f64 inside.
#include <math.h>

#include "common.h"

namespace {

constexpr int kVolMaxViews = 8;
constexpr int kVolThreads = 256;
constexpr int kVolChunk = 8;             // channels per thread of the forward
constexpr int kVolBwdThreads = 512;
constexpr int kVolBwdMaxCh = 4;          // planes per workgroup of the backward
constexpr size_t kVolBwdLds = 128 * 1024;   // bytes of fixed-point planes per workgroup (of the 160 KB)
constexpr int kVolSplit = HR_VOLUME_SPLIT;  // workgroups per map of the integrate launches
constexpr double kVolMagic = 6755399441055744.0;   // 1.5 * 2^52

enum { kSum = HR_VOL_SUM, kMax = HR_VOL_MAX, kSoftmax = HR_VOL_SOFTMAX, kConf = HR_VOL_CONF };

struct VolPos {
  int i00;          // y0 * W + x0 (any value when mask == 0)
  float wx, wy;     // weights of column x0 + 1 and row y0 + 1
  unsigned mask;    // bit 0: (y0, x0), 1: (y0, x0 + 1), 2: (y0 + 1, x0), 3: (y0 + 1, x0 + 1) inside the map
};

__device__ __forceinline__ VolPos vol_position(const float* __restrict__ P, double px, double py, double pz, int H,
                                               int W) {
  const double qx = fma((double)P[0], px, fma((double)P[1], py, fma((double)P[2], pz, (double)P[3])));
  const double qy = fma((double)P[4], px, fma((double)P[5], py, fma((double)P[6], pz, (double)P[7])));
  const double qz = fma((double)P[8], px, fma((double)P[9], py, fma((double)P[10], pz, (double)P[11])));
  VolPos r;
  r.i00 = 0;
  r.wx = 0.f;
  r.wy = 0.f;
  r.mask = 0u;
  // invalid view: the sample is 0 whatever the position (so the reference's q.z == 0 -> 1 needs no divide here)
  if (qz <= 0.0) return r;
  const double ix = (qx / qz) * (double)(W - 1) / (double)H;
  const double iy = (qy / qz) * (double)(H - 1) / (double)W;
  // all four corners outside (NaN positions included): nothing is read
  if (!(ix > -1.0 && ix < (double)W && iy > -1.0 && iy < (double)H)) return r;
  const double fx = floor(ix), fy = floor(iy);
  const int x0 = (int)fx, y0 = (int)fy;         // -1 .. W - 1, -1 .. H - 1
  r.wx = (float)(ix - fx);
  r.wy = (float)(iy - fy);
  const bool xa = x0 >= 0, xb = x0 + 1 <= W - 1, ya = y0 >= 0, yb = y0 + 1 <= H - 1;
  r.mask = (ya && xa ? 1u : 0u) | (ya && xb ? 2u : 0u) | (yb && xa ? 4u : 0u) | (yb && xb ? 8u : 0u);
  r.i00 = y0 * W + x0;
  return r;
}

__device__ __forceinline__ float vol_sample(const float* __restrict__ plane, const VolPos& p, int W) {
  if (p.mask == 0u) return 0.f;
  const float v00 = p.mask & 1u ? plane[p.i00] : 0.f;
  const float v01 = p.mask & 2u ? plane[p.i00 + 1] : 0.f;
  const float v10 = p.mask & 4u ? plane[p.i00 + W] : 0.f;
  const float v11 = p.mask & 8u ? plane[p.i00 + W + 1] : 0.f;
  const float ax = 1.f - p.wx, ay = 1.f - p.wy;
  return v00 * (ax * ay) + v01 * (p.wx * ay) + v10 * (ax * p.wy) + v11 * (p.wx * p.wy);
}

// the V samples of one (channel, voxel) -> the aggregated value
template <int METHOD>
__device__ __forceinline__ float vol_aggregate(const float (&s)[kVolMaxViews], const float (&cw)[kVolMaxViews],
                                               int V) {
  float out = 0.f;
  if (METHOD == kSum) {
#pragma unroll
    for (int v = 0; v < kVolMaxViews; ++v)
      if (v < V) out += s[v];
  } else if (METHOD == kConf) {
#pragma unroll
    for (int v = 0; v < kVolMaxViews; ++v)
      if (v < V) out += cw[v] * s[v];
  } else if (METHOD == kMax) {
    out = s[0];
#pragma unroll
    for (int v = 1; v < kVolMaxViews; ++v)
      if (v < V && s[v] > out) out = s[v];
  } else {
    float m = s[0];
#pragma unroll
    for (int v = 1; v < kVolMaxViews; ++v)
      if (v < V) m = fmaxf(m, s[v]);
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int v = 0; v < kVolMaxViews; ++v)
      if (v < V) {
        const float e = expf(s[v] - m);
        den += e;
        num += s[v] * e;
      }
    out = num / den;
  }
  return out;
}

template <int METHOD>
__global__ __launch_bounds__(kVolThreads) void unproject_fwd_kernel(const float* __restrict__ feat,
                                                                    const float* __restrict__ proj,
                                                                    const float* __restrict__ coord,
                                                                    const float* __restrict__ conf,
                                                                    float* __restrict__ vol, int V, int C, int H, int W,
                                                                    long long nvox) {
  const long long n = (long long)blockIdx.x * kVolThreads + threadIdx.x;
  if (n >= nvox) return;
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * kVolChunk;
  const int c1 = c0 + kVolChunk < C ? c0 + kVolChunk : C;
  const float* cp = coord + ((long long)b * nvox + n) * 3;
  const double px = (double)cp[0], py = (double)cp[1], pz = (double)cp[2];
  VolPos pos[kVolMaxViews];
#pragma unroll
  for (int v = 0; v < kVolMaxViews; ++v)
    if (v < V) pos[v] = vol_position(proj + ((long long)b * V + v) * 12, px, py, pz, H, W);
  const long long HW = (long long)H * W;
  for (int c = c0; c < c1; ++c) {
    float s[kVolMaxViews], cw[kVolMaxViews];
#pragma unroll
    for (int v = 0; v < kVolMaxViews; ++v) {
      s[v] = 0.f;
      cw[v] = 0.f;
      if (v < V) {
        const long long slot = ((long long)b * V + v) * C + c;
        s[v] = vol_sample(feat + slot * HW, pos[v], W);
        if (METHOD == kConf) cw[v] = conf[slot];
      }
    }
    vol[((long long)b * C + c) * nvox + n] = vol_aggregate<METHOD>(s, cw, V);
  }
}

// largest |x| of n values over the workgroup (every thread gets it); `bad` is set when a value is not finite
__device__ __forceinline__ float vol_block_absmax(const float* __restrict__ x, long long n, float* red, int* bad) {
  float m = 0.f;
  int nf = 0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const float a = fabsf(x[i]);
    if (!(a <= 3.0e38f)) nf = 1;
    m = fmaxf(m, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
    nf |= __shfl_xor(nf, o);
  }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();                        // red is free
  if ((threadIdx.x & 63) == 0) {
    red[wave] = m;
    red[16 + wave] = nf ? 1.f : 0.f;
  }
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < nw; ++w) {
    r = fmaxf(r, red[w]);
    if (red[16 + w] != 0.f) *bad = 1;
  }
  return r;
}

template <int METHOD>
__global__ __launch_bounds__(kVolBwdThreads) void unproject_bwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ proj, const float* __restrict__ coord,
    const float* __restrict__ conf, const float* __restrict__ gV, float* __restrict__ dfeat, float* __restrict__ dconf,
    int V, int C, int H, int W, long long nvox, int CH) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long planes[];   // [CH][H * W], 64-bit fixed point
  __shared__ float red[32];
  __shared__ double dred[kVolBwdThreads / 64];
  __shared__ double fscale_s[kVolBwdMaxCh], funscale_s[kVolBwdMaxCh];
  __shared__ int bad_s[kVolBwdMaxCh];
  const int HW = H * W;
  const int c0 = blockIdx.x * CH, v_own = blockIdx.y, b = blockIdx.z;
  const int nch = c0 + CH <= C ? CH : C - c0;
  for (int i = threadIdx.x; i < nch * HW; i += kVolBwdThreads) planes[i] = 0ull;
  int cells_log = 0;
  while ((1ll << cells_log) < nvox) ++cells_log;        // a cell receives at most one share per voxel
  for (int k = 0; k < nch; ++k) {
    const int c = c0 + k;
    int bad = 0;
    const float gmax = vol_block_absmax(gV + ((long long)b * C + c) * nvox, nvox, red, &bad);
    float fmax = 1.f;
    if (METHOD == kConf) {
      fmax = fabsf(conf[((long long)b * V + v_own) * C + c]);
      if (!(fmax <= 3.0e38f)) bad = 1;
    }
    if (METHOD == kSoftmax) {
      float xmax = 0.f;
      for (int v = 0; v < V; ++v)
        xmax = fmaxf(xmax, vol_block_absmax(feat + (((long long)b * V + v) * C + c) * HW, HW, red, &bad));
      fmax = 1.f + 2.f * xmax;
    }
    const float bound = gmax * fmax;                    // >= |factor * gV| of every voxel of this plane
    if (!(bound <= 3.0e38f)) bad = 1;
    int bx = 0;
    (void)frexpf(!bad && bound > 0.f ? bound : 1.f, &bx);          // bound < 2^bx
    const int fe = (50 < 61 - cells_log ? 50 : 61 - cells_log) - bx;
    if (threadIdx.x == 0) {
      fscale_s[k] = ldexp(1.0, fe);
      funscale_s[k] = ldexp(1.0, -fe);
      bad_s[k] = bad;
    }
  }
  __syncthreads();               // zeroed planes and the scales are complete
  double dc_acc[kVolBwdMaxCh] = {0.0, 0.0, 0.0, 0.0};
  for (long long n = threadIdx.x; n < nvox; n += kVolBwdThreads) {
    const float* cp = coord + ((long long)b * nvox + n) * 3;
    const double px = (double)cp[0], py = (double)cp[1], pz = (double)cp[2];
    VolPos pos[kVolMaxViews];
    if (METHOD == kSum || METHOD == kConf) {
      pos[0] = vol_position(proj + ((long long)b * V + v_own) * 12, px, py, pz, H, W);
      if (pos[0].mask == 0u && METHOD == kSum) continue;
    } else {
#pragma unroll
      for (int v = 0; v < kVolMaxViews; ++v)
        if (v < V) pos[v] = vol_position(proj + ((long long)b * V + v) * 12, px, py, pz, H, W);
    }
#pragma unroll
    for (int k = 0; k < kVolBwdMaxCh; ++k) {
      if (k >= nch) break;
      const int c = c0 + k;
      const float g = gV[((long long)b * C + c) * nvox + n];
      float factor = 1.f;
      VolPos own = pos[0];
      if (METHOD == kConf) {
        const long long slot = ((long long)b * V + v_own) * C + c;
        factor = conf[slot];
        if (dconf) dc_acc[k] += (double)(g * vol_sample(feat + slot * HW, own, W));
      }
      if (METHOD == kMax || METHOD == kSoftmax) {
        float s[kVolMaxViews];
#pragma unroll
        for (int v = 0; v < kVolMaxViews; ++v) {
          s[v] = 0.f;
          if (v < V) s[v] = vol_sample(feat + (((long long)b * V + v) * C + c) * HW, pos[v], W);
        }
        float s_own = 0.f;
#pragma unroll
        for (int v = 0; v < kVolMaxViews; ++v)
          if (v == v_own) {
            own = pos[v];
            s_own = s[v];
          }
        if (METHOD == kMax) {
          int win = 0;
          float best = s[0];
#pragma unroll
          for (int v = 1; v < kVolMaxViews; ++v)
            if (v < V && s[v] > best) {
              best = s[v];
              win = v;
            }
          factor = win == v_own ? 1.f : 0.f;
        } else {
          float m = s[0];
#pragma unroll
          for (int v = 1; v < kVolMaxViews; ++v)
            if (v < V) m = fmaxf(m, s[v]);
          float den = 0.f, num = 0.f;
#pragma unroll
          for (int v = 0; v < kVolMaxViews; ++v)
            if (v < V) {
              const float e = expf(s[v] - m);
              den += e;
              num += s[v] * e;
            }
          const float sm = expf(s_own - m) / den;
          factor = sm * (1.f + s_own - num / den);
        }
      }
      if (own.mask == 0u) continue;
      const double gs = (double)(g * factor) * fscale_s[k];
      unsigned long long* pl = planes + (size_t)k * HW;
      const float ax = 1.f - own.wx, ay = 1.f - own.wy;
      auto add = [&](int cell, float w) {
        const double d = __builtin_fma(gs, (double)w, kVolMagic);
        const unsigned long long q =
            (unsigned long long)(__builtin_bit_cast(long long, d) - __builtin_bit_cast(long long, kVolMagic));
        __hip_atomic_fetch_add(pl + cell, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      };
      if (own.mask & 1u) add(own.i00, ax * ay);
      if (own.mask & 2u) add(own.i00 + 1, own.wx * ay);
      if (own.mask & 4u) add(own.i00 + W, ax * own.wy);
      if (own.mask & 8u) add(own.i00 + W + 1, own.wx * own.wy);
    }
  }
  __syncthreads();               // every share is in the planes
  for (int k = 0; k < nch; ++k) {
    float* out = dfeat + (((long long)b * V + v_own) * C + c0 + k) * HW;
    const double un = funscale_s[k];
    const bool finite = bad_s[k] == 0;
    const unsigned long long* pl = planes + (size_t)k * HW;
    for (int i = threadIdx.x; i < HW; i += kVolBwdThreads)
      out[i] = finite ? (float)((double)(long long)pl[i] * un) : __builtin_nanf("");
  }
  if (METHOD == kConf && dconf) {
    // f64 partials per thread, summed over the wave by a fixed butterfly and over the waves in index order
    for (int k = 0; k < nch; ++k) {
      double a = dc_acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
      __syncthreads();
      if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = a;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kVolBwdThreads / 64; ++w) t += dred[w];
        dconf[((long long)b * V + v_own) * C + c0 + k] = (float)t;
      }
    }
  }
}

// ---- 3-D soft-argmax ------------------------------------------------------------------------------------------------

// sum of `a` over the workgroup in a fixed order (butterfly in the wave, waves in index order); every thread gets it
__device__ __forceinline__ double vol_block_sum(double a, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

__device__ __forceinline__ void vol_chunk(long long nvox, long long& lo, long long& hi) {
  const long long len = (nvox + kVolSplit - 1) / kVolSplit;
  lo = (long long)blockIdx.x * len;
  hi = lo + len < nvox ? lo + len : nvox;
  if (lo > nvox) lo = nvox;
}

// partials [B*J][kVolSplit][5] f64: (max of multiplier * x, sum exp(. - max), three moments) of the chunk; relu mode:
// (0, 0, three moments of relu(multiplier * x))
__global__ __launch_bounds__(kVolThreads) void integrate_partial_kernel(const float* __restrict__ vols,
                                                                        const float* __restrict__ coord,
                                                                        double* __restrict__ work, double mult,
                                                                        int softmax, int J, long long nvox) {
  __shared__ double red[kVolThreads / 64];
  const long long map = blockIdx.y, b = map / J;
  long long lo, hi;
  vol_chunk(nvox, lo, hi);
  const float* x = vols + map * nvox;
  const float* cv = coord + b * nvox * 3;
  double m = 0.0;
  if (softmax) {
    m = -INFINITY;
    for (long long i = lo + threadIdx.x; i < hi; i += kVolThreads) m = fmax(m, mult * (double)x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < kVolThreads / 64; ++w) m = fmax(m, red[w]);
  }
  double s = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kVolThreads) {
    const double t = mult * (double)x[i];
    const double e = softmax ? exp(t - m) : (t > 0.0 ? t : 0.0);
    s += e;
    mx += e * (double)cv[3 * i];
    my += e * (double)cv[3 * i + 1];
    mz += e * (double)cv[3 * i + 2];
  }
  s = vol_block_sum(s, red);
  mx = vol_block_sum(mx, red);
  my = vol_block_sum(my, red);
  mz = vol_block_sum(mz, red);
  if (threadIdx.x == 0) {
    double* w = work + (map * kVolSplit + blockIdx.x) * 5;
    w[0] = m;
    w[1] = softmax ? s : 0.0;
    w[2] = mx;
    w[3] = my;
    w[4] = mz;
  }
}

__global__ __launch_bounds__(kVolThreads) void integrate_final_kernel(const float* __restrict__ vols,
                                                                      const double* __restrict__ work,
                                                                      float* __restrict__ keypoints,
                                                                      float* __restrict__ p, double mult, int softmax,
                                                                      long long nvox) {
  const long long map = blockIdx.y;
  long long lo, hi;
  vol_chunk(nvox, lo, hi);
  const double* w = work + map * kVolSplit * 5;
  // every workgroup of the map merges the same partials in the same order
  double M = 0.0, total = 1.0, kx = 0.0, ky = 0.0, kz = 0.0;
  if (softmax) {
    M = -INFINITY;
    for (int k = 0; k < kVolSplit; ++k) M = fmax(M, w[5 * k]);
    total = 0.0;
    for (int k = 0; k < kVolSplit; ++k) {
      if (w[5 * k + 1] == 0.0) continue;                 // an empty chunk (its max is -inf)
      const double f = exp(w[5 * k] - M);
      total += w[5 * k + 1] * f;
      kx += w[5 * k + 2] * f;
      ky += w[5 * k + 3] * f;
      kz += w[5 * k + 4] * f;
    }
  } else {
    for (int k = 0; k < kVolSplit; ++k) {
      kx += w[5 * k + 2];
      ky += w[5 * k + 3];
      kz += w[5 * k + 4];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    keypoints[3 * map] = (float)(kx / total);
    keypoints[3 * map + 1] = (float)(ky / total);
    keypoints[3 * map + 2] = (float)(kz / total);
  }
  const float* x = vols + map * nvox;
  float* out = p + map * nvox;
  for (long long i = lo + threadIdx.x; i < hi; i += kVolThreads) {
    const double t = mult * (double)x[i];
    out[i] = (float)(softmax ? exp(t - M) / total : (t > 0.0 ? t : 0.0));
  }
}

// softmax backward, first launch: partial sums of p_i t_i, t_i = gK . coord_i + gP_i, work [B*J][kVolSplit] f64
__global__ __launch_bounds__(kVolThreads) void integrate_bwd_partial_kernel(const float* __restrict__ p,
                                                                            const float* __restrict__ coord,
                                                                            const float* __restrict__ gK,
                                                                            const float* __restrict__ gP,
                                                                            double* __restrict__ work, int J,
                                                                            long long nvox) {
  __shared__ double red[kVolThreads / 64];
  const long long map = blockIdx.y, b = map / J;
  long long lo, hi;
  vol_chunk(nvox, lo, hi);
  const float* cv = coord + b * nvox * 3;
  const double g0 = (double)gK[3 * map], g1 = (double)gK[3 * map + 1], g2 = (double)gK[3 * map + 2];
  double s = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kVolThreads) {
    double t = g0 * (double)cv[3 * i] + g1 * (double)cv[3 * i + 1] + g2 * (double)cv[3 * i + 2];
    if (gP) t += (double)gP[map * nvox + i];
    s += (double)p[map * nvox + i] * t;
  }
  s = vol_block_sum(s, red);
  if (threadIdx.x == 0) work[map * kVolSplit + blockIdx.x] = s;
}

__global__ __launch_bounds__(kVolThreads) void integrate_bwd_final_kernel(
    const float* __restrict__ vols, const float* __restrict__ p, const float* __restrict__ coord,
    const float* __restrict__ gK, const float* __restrict__ gP, const double* __restrict__ work,
    float* __restrict__ dvols, double mult, int softmax, int J, long long nvox) {
  const long long map = blockIdx.y, b = map / J;
  long long lo, hi;
  vol_chunk(nvox, lo, hi);
  const float* cv = coord + b * nvox * 3;
  const double g0 = (double)gK[3 * map], g1 = (double)gK[3 * map + 1], g2 = (double)gK[3 * map + 2];
  double dot = 0.0;
  if (softmax)
    for (int k = 0; k < kVolSplit; ++k) dot += work[map * kVolSplit + k];
  for (long long i = lo + threadIdx.x; i < hi; i += kVolThreads) {
    double t = g0 * (double)cv[3 * i] + g1 * (double)cv[3 * i + 1] + g2 * (double)cv[3 * i + 2];
    if (gP) t += (double)gP[map * nvox + i];
    double d;
    if (softmax)
      d = mult * (double)p[map * nvox + i] * (t - dot);
    else
      d = mult * (double)vols[map * nvox + i] > 0.0 ? mult * t : 0.0;
    dvols[map * nvox + i] = (float)d;
  }
}

// ---- volumetric cross-entropy ---------------------------------------------------------------------------------------

// one workgroup per (b, j): the voxel nearest gt[b, j], f64 squared distances, the first of equal distances wins
__global__ __launch_bounds__(kVolThreads) void ce_nearest_kernel(const float* __restrict__ coord,
                                                                 const float* __restrict__ gt, int* __restrict__ idx,
                                                                 int J, long long nvox) {
  __shared__ double dmin[kVolThreads];
  __shared__ long long imin[kVolThreads];
  const long long map = blockIdx.x, b = map / J;
  const float* cv = coord + b * nvox * 3;
  const double gx = (double)gt[3 * map], gy = (double)gt[3 * map + 1], gz = (double)gt[3 * map + 2];
  double best = INFINITY;
  long long bi = nvox;                       // nvox: nothing compared below `best` yet (NaN distances)
  for (long long i = threadIdx.x; i < nvox; i += kVolThreads) {
    const double dx = (double)cv[3 * i] - gx, dy = (double)cv[3 * i + 1] - gy, dz = (double)cv[3 * i + 2] - gz;
    const double d = dx * dx + dy * dy + dz * dz;
    if (d < best) {                          // ascending i per thread: the first of equals stays
      best = d;
      bi = i;
    }
  }
  dmin[threadIdx.x] = best;
  imin[threadIdx.x] = bi;
  __syncthreads();
  for (int o = kVolThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double d2 = dmin[threadIdx.x + o];
      const long long i2 = imin[threadIdx.x + o];
      if (d2 < dmin[threadIdx.x] || (d2 == dmin[threadIdx.x] && i2 < imin[threadIdx.x])) {
        dmin[threadIdx.x] = d2;
        imin[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) idx[map] = (int)(imin[0] < nvox ? imin[0] : 0);
}

// one workgroup: loss = sum_{b,j} validity (-log(p[idx] + 1e-6)) / (B J), f64, fixed order
__global__ __launch_bounds__(kVolThreads) void ce_loss_kernel(const float* __restrict__ p,
                                                              const float* __restrict__ validity,
                                                              const int* __restrict__ idx, float* __restrict__ loss,
                                                              long long maps, long long nvox) {
  __shared__ double red[kVolThreads / 64];
  double s = 0.0;
  for (long long i = threadIdx.x; i < maps; i += kVolThreads) {
    const double v = (double)validity[i];
    if ((unsigned)idx[i] >= nvox) continue;              // never from ce_nearest_kernel
    s += v * -log((double)p[i * nvox + idx[i]] + 1e-6);
  }
  s = vol_block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)maps);
}

__global__ __launch_bounds__(kVolThreads) void ce_loss_bwd_kernel(const float* __restrict__ p,
                                                                  const float* __restrict__ validity,
                                                                  const int* __restrict__ idx,
                                                                  const float* __restrict__ gout,
                                                                  float* __restrict__ dp, long long maps,
                                                                  long long nvox) {
  const long long i = (long long)blockIdx.x * kVolThreads + threadIdx.x;
  if (i >= maps || (unsigned)idx[i] >= nvox) return;     // an index outside the map is not written
  const long long at = i * nvox + idx[i];
  dp[at] = (float)(-(double)gout[0] * (double)validity[i] / ((double)p[at] + 1e-6) / (double)maps);
}

// dynamic LDS beyond the default window has to be granted per kernel: once, on the first backward call of the process
// (whatever its size, so that the call never falls into a later stream capture), and checked
int vol_bwd_grant_lds() {
  static bool granted = false;
  if (granted) return HR_OK;
  const void* kernels[4] = {(const void*)unproject_bwd_kernel<kSum>, (const void*)unproject_bwd_kernel<kMax>,
                            (const void*)unproject_bwd_kernel<kSoftmax>, (const void*)unproject_bwd_kernel<kConf>};
  for (const void* k : kernels)
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVolBwdLds) != hipSuccess) {
      hr_set_error("unproject_volume_bwd: hipFuncSetAttribute(%d bytes of dynamic LDS) failed", (int)kVolBwdLds);
      return HR_E_LAUNCH;
    }
  granted = true;
  return HR_OK;
}

int vol_check_unproject(const char* what, int method, const void* conf, int B, int V, int C, int H, int W, int X, int Y,
                        int Z) {
  HR_REQUIRE(method >= kSum && method <= kConf, "%s: method = %d (0 sum, 1 max, 2 softmax, 3 conf)", what, method);
  HR_REQUIRE(method != kConf || conf, "%s: the conf method needs confidences", what);
  HR_REQUIRE(V >= 1 && V <= kVolMaxViews, "%s: V = %d views (1..%d)", what, V, kVolMaxViews);
  HR_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && H >= 1 && W >= 1 && X >= 1 && Y >= 1 && Z >= 1,
             "%s: B = %d (1..65535), C = %d, H = %d, W = %d, X = %d, Y = %d, Z = %d", what, B, C, H, W, X, Y, Z);
  HR_REQUIRE((long long)H * W <= HR_VOLUME_MAX_MAP, "%s: H * W = %lld pixels (at most %d)", what, (long long)H * W,
             HR_VOLUME_MAX_MAP);
  HR_REQUIRE((long long)X * Y * Z <= (1LL << 30), "%s: X * Y * Z = %lld voxels (at most 2^30)", what,
             (long long)X * Y * Z);
  HR_REQUIRE((C + kVolChunk - 1) / kVolChunk <= 65535 && (long long)V * C <= (1LL << 24), "%s: C = %d channels", what,
             C);
  return HR_OK;
}

int vol_check_maps(const char* what, int B, int J, int X, int Y, int Z) {
  HR_REQUIRE(B >= 1 && J >= 1 && X >= 1 && Y >= 1 && Z >= 1 && (long long)B * J <= 65535,
             "%s: B = %d, J = %d (B * J at most 65535), X = %d, Y = %d, Z = %d", what, B, J, X, Y, Z);
  HR_REQUIRE((long long)X * Y * Z <= (1LL << 30), "%s: X * Y * Z = %lld voxels (at most 2^30)", what,
             (long long)X * Y * Z);
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_unproject_volume(const float* features, const float* proj, const float* coord, const float* conf,
                                      float* volumes, int method, int B, int V, int C, int H, int W, int X, int Y,
                                      int Z, hr_stream_t stream) {
  HR_REQUIRE(features && proj && coord && volumes, "unproject_volume: null argument");
  const int rc = vol_check_unproject("unproject_volume", method, conf, B, V, C, H, W, X, Y, Z);
  if (rc != HR_OK) return rc;
  const long long nvox = (long long)X * Y * Z;
  const dim3 grid((unsigned)((nvox + kVolThreads - 1) / kVolThreads), (unsigned)((C + kVolChunk - 1) / kVolChunk),
                  (unsigned)B);
#define VOL_FWD(M)                                                                                                   \
  hipLaunchKernelGGL(unproject_fwd_kernel<M>, grid, dim3(kVolThreads), 0, (hipStream_t)stream, features, proj, coord, \
                     conf, volumes, V, C, H, W, nvox)
  switch (method) {
    case kSum: VOL_FWD(kSum); break;
    case kMax: VOL_FWD(kMax); break;
    case kSoftmax: VOL_FWD(kSoftmax); break;
    default: VOL_FWD(kConf); break;
  }
#undef VOL_FWD
  return hr_check_launch("unproject_volume");
}

extern "C" int hrnet_unproject_volume_bwd(const float* features, const float* proj, const float* coord,
                                          const float* conf, const float* gV, float* dfeatures, float* dconf,
                                          int method, int B, int V, int C, int H, int W, int X, int Y, int Z,
                                          hr_stream_t stream) {
  HR_REQUIRE(features && proj && coord && gV && dfeatures, "unproject_volume_bwd: null argument");
  const int rc = vol_check_unproject("unproject_volume_bwd", method, conf, B, V, C, H, W, X, Y, Z);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(method == kConf || !dconf, "unproject_volume_bwd: dconf is for the conf method only");
  const long long nvox = (long long)X * Y * Z;
  const size_t plane = (size_t)H * W * sizeof(unsigned long long);
  // planes per workgroup: what the LDS holds, fewer while that leaves under ~2 workgroups per compute unit
  int CH = (int)(kVolBwdLds / plane);
  if (CH > kVolBwdMaxCh) CH = kVolBwdMaxCh;
  if (CH > C) CH = C;
  while (CH > 1 && (long long)B * V * ((C + CH - 1) / CH) < 512) --CH;
  const dim3 grid((unsigned)((C + CH - 1) / CH), (unsigned)V, (unsigned)B);
  const size_t lds = plane * CH;
  const int rg = vol_bwd_grant_lds();
  if (rg != HR_OK) return rg;
#define VOL_BWD(M)                                                                                              \
  hipLaunchKernelGGL(unproject_bwd_kernel<M>, grid, dim3(kVolBwdThreads), lds, (hipStream_t)stream, features, \
                     proj, coord, conf, gV, dfeatures, dconf, V, C, H, W, nvox, CH)
  switch (method) {
    case kSum: VOL_BWD(kSum); break;
    case kMax: VOL_BWD(kMax); break;
    case kSoftmax: VOL_BWD(kSoftmax); break;
    default: VOL_BWD(kConf); break;
  }
#undef VOL_BWD
  return hr_check_launch("unproject_volume_bwd");
}

extern "C" int hrnet_volume_integrate(const float* vols, const float* coord, float multiplier, int softmax,
                                      float* keypoints, float* p, double* work, int B, int J, int X, int Y, int Z,
                                      hr_stream_t stream) {
  HR_REQUIRE(vols && coord && keypoints && p && work, "volume_integrate: null argument");
  const int rc = vol_check_maps("volume_integrate", B, J, X, Y, Z);
  if (rc != HR_OK) return rc;
  const long long nvox = (long long)X * Y * Z;
  const dim3 grid(kVolSplit, (unsigned)(B * J));
  hipLaunchKernelGGL(integrate_partial_kernel, grid, dim3(kVolThreads), 0, (hipStream_t)stream, vols, coord, work,
                     (double)multiplier, softmax ? 1 : 0, J, nvox);
  hipLaunchKernelGGL(integrate_final_kernel, grid, dim3(kVolThreads), 0, (hipStream_t)stream, vols, work, keypoints, p,
                     (double)multiplier, softmax ? 1 : 0, nvox);
  return hr_check_launch("volume_integrate");
}

extern "C" int hrnet_volume_integrate_bwd(const float* vols, const float* p, const float* coord, const float* gK,
                                          const float* gP, float multiplier, int softmax, float* dvols, double* work,
                                          int B, int J, int X, int Y, int Z, hr_stream_t stream) {
  HR_REQUIRE(vols && p && coord && gK && dvols && work, "volume_integrate_bwd: null argument");
  const int rc = vol_check_maps("volume_integrate_bwd", B, J, X, Y, Z);
  if (rc != HR_OK) return rc;
  const long long nvox = (long long)X * Y * Z;
  const dim3 grid(kVolSplit, (unsigned)(B * J));
  if (softmax)
    hipLaunchKernelGGL(integrate_bwd_partial_kernel, grid, dim3(kVolThreads), 0, (hipStream_t)stream, p, coord, gK, gP,
                       work, J, nvox);
  hipLaunchKernelGGL(integrate_bwd_final_kernel, grid, dim3(kVolThreads), 0, (hipStream_t)stream, vols, p, coord, gK,
                     gP, work, dvols, (double)multiplier, softmax ? 1 : 0, J, nvox);
  return hr_check_launch("volume_integrate_bwd");
}

extern "C" int hrnet_volumetric_ce_loss(const float* coord, const float* p, const float* gt, const float* validity,
                                        float* loss, int* idx, int B, int J, int X, int Y, int Z,
                                        hr_stream_t stream) {
  HR_REQUIRE(coord && p && gt && validity && loss && idx, "volumetric_ce_loss: null argument");
  const int rc = vol_check_maps("volumetric_ce_loss", B, J, X, Y, Z);
  if (rc != HR_OK) return rc;
  const long long nvox = (long long)X * Y * Z, maps = (long long)B * J;
  hipLaunchKernelGGL(ce_nearest_kernel, dim3((unsigned)maps), dim3(kVolThreads), 0, (hipStream_t)stream, coord, gt, idx,
                     J, nvox);
  hipLaunchKernelGGL(ce_loss_kernel, dim3(1), dim3(kVolThreads), 0, (hipStream_t)stream, p, validity, idx, loss, maps,
                     nvox);
  return hr_check_launch("volumetric_ce_loss");
}

extern "C" int hrnet_volumetric_ce_loss_bwd(const float* p, const float* validity, const int* idx, const float* gout,
                                            float* dp, int B, int J, int X, int Y, int Z, hr_stream_t stream) {
  HR_REQUIRE(p && validity && idx && gout && dp, "volumetric_ce_loss_bwd: null argument");
  const int rc = vol_check_maps("volumetric_ce_loss_bwd", B, J, X, Y, Z);
  if (rc != HR_OK) return rc;
  const long long nvox = (long long)X * Y * Z, maps = (long long)B * J;
  const int rz = hrnet_fill_zero(dp, (int64_t)(maps * nvox * (long long)sizeof(float)), stream);
  if (rz != HR_OK) return rz;
  hipLaunchKernelGGL(ce_loss_bwd_kernel, dim3((unsigned)((maps + kVolThreads - 1) / kVolThreads)), dim3(kVolThreads), 0,
                     (hipStream_t)stream, p, validity, idx, gout, dp, maps, nvox);
  return hr_check_launch("volumetric_ce_loss_bwd");
}
