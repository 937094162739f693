// The burger's glue of pose_hrnet_hamburger in training mode (reference lib/models/hamburger/burger.py:198-199 and the
// Dropout2d of lib/models/pose_hrnet_hamburger.py:62): out = relu(coef_ham * u + coef_shortcut * s) with its backward
// (two map gradients and the two scalar ones in ONE pass), and Dropout2d on a given keep mask.
//
// Streaming kernels on f32 NHWC rows [rows][C], C % 16 == 0, 64-bit element offsets. A grid is sized to the device (a
// fixed number of workgroups, a function of the shape alone) and strides over the map; four floats per lane and access
// when every map pointer is 16-byte aligned, one float otherwise, in the same kernel. No atomics: the scalar sums are
// made in double per thread, added over the workgroup in a fixed order, stored as per-workgroup partials and added in
// index order by a second launch, so a call is bit-reproducible.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMixBlocks = 1024;        // 256 CUs x 4 workgroups of 256 threads
constexpr int kBwdBlocks = 512;         // the partials of the two sums: 2 x 512 doubles, added serially from LDS
constexpr long long kMaxElems = 1LL << 40;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int blocks_for(long long n, int per_thread, int cap) {
  const long long work = (n + (long long)kThreads * per_thread - 1) / ((long long)kThreads * per_thread);
  return (int)(work < cap ? (work < 1 ? 1 : work) : cap);
}

inline bool shape_ok(long long rows, int C) {
  return rows >= 1 && C >= 16 && C % 16 == 0 && rows <= kMaxElems / C;
}

__device__ __forceinline__ float mix1(float u, float s, float ch, float cs) { return fmaxf(fmaf(ch, u, cs * s), 0.f); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void burger_mix_kernel(const float* u, const float* s, const float* coef_ham,
                                                              const float* coef_shortcut, float* out, long long n) {
  const float ch = *coef_ham, cs = *coef_shortcut;
  const long long stride = (long long)gridDim.x * kThreads;
  long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (VEC) {
    const long long n4 = n >> 2;                    // C % 16 == 0: nothing is left over
    const f32x4* u4 = (const f32x4*)u;
    const f32x4* s4 = (const f32x4*)s;
    f32x4* o4 = (f32x4*)out;
    for (; i < n4; i += stride) {
      const f32x4 a = u4[i], b = s4[i];
      o4[i] = f32x4{mix1(a.x, b.x, ch, cs), mix1(a.y, b.y, ch, cs), mix1(a.z, b.z, ch, cs), mix1(a.w, b.w, ch, cs)};
    }
  } else {
    for (; i < n; i += stride) out[i] = mix1(u[i], s[i], ch, cs);
  }
}

__device__ __forceinline__ void bwd1(float g, float o, float u, float s, float ch, float cs, float& du, float& ds,
                                     double& su, double& ss) {
  const float gm = o > 0.f ? g : 0.f;
  du = ch * gm;
  ds = cs * gm;
  su = fma((double)gm, (double)u, su);
  ss = fma((double)gm, (double)s, ss);
}

__device__ __forceinline__ double wave_sum64d(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void burger_mix_bwd_kernel(const float* g, const float* out, const float* u,
                                                                  const float* s, const float* coef_ham,
                                                                  const float* coef_shortcut, float* du, float* ds,
                                                                  double* partials, long long n) {
  __shared__ double red[2][kThreads / 64];
  const float ch = *coef_ham, cs = *coef_shortcut;
  const long long stride = (long long)gridDim.x * kThreads;
  long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  double su = 0.0, ss = 0.0;
  if (VEC) {
    const long long n4 = n >> 2;
    for (; i < n4; i += stride) {
      const f32x4 a = ((const f32x4*)g)[i], o = ((const f32x4*)out)[i], b = ((const f32x4*)u)[i], c = ((const f32x4*)s)[i];
      float x[4], y[4];
      bwd1(a.x, o.x, b.x, c.x, ch, cs, x[0], y[0], su, ss);
      bwd1(a.y, o.y, b.y, c.y, ch, cs, x[1], y[1], su, ss);
      bwd1(a.z, o.z, b.z, c.z, ch, cs, x[2], y[2], su, ss);
      bwd1(a.w, o.w, b.w, c.w, ch, cs, x[3], y[3], su, ss);
      if (du) ((f32x4*)du)[i] = f32x4{x[0], x[1], x[2], x[3]};
      if (ds) ((f32x4*)ds)[i] = f32x4{y[0], y[1], y[2], y[3]};
    }
  } else {
    for (; i < n; i += stride) {
      float x, y;
      bwd1(g[i], out[i], u[i], s[i], ch, cs, x, y, su, ss);
      if (du) du[i] = x;
      if (ds) ds[i] = y;
    }
  }
  if (!partials) return;
  su = wave_sum64d(su);
  ss = wave_sum64d(ss);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = su;
    red[1][wave] = ss;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) t += red[threadIdx.x][w];
    partials[2 * (long long)blockIdx.x + threadIdx.x] = t;
  }
}

// one workgroup: the partials go through LDS, then thread 0 adds those of sum gm * u and thread 64 (another wave) those
// of sum gm * s, each in workgroup order
__global__ __launch_bounds__(kThreads) void burger_mix_reduce_kernel(const double* partials, int blocks, float* dcoef) {
  __shared__ double stage[2 * kBwdBlocks];
  for (int i = threadIdx.x; i < 2 * blocks; i += kThreads) stage[i] = partials[i];
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {
    const int which = threadIdx.x >> 6;
    double t = 0.0;
    for (int b = 0; b < blocks; ++b) t += stage[2 * b + which];
    dcoef[which] = (float)t;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void dropout2d_kernel(const float* x, const float* keep, float* y, long long n,
                                                             long long P, int C) {
  const long long stride = (long long)gridDim.x * kThreads;
  long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool small = n <= 0x7fffffffLL;              // 32-bit divisions where the element index fits
  if (VEC) {
    const long long n4 = n >> 2;
    const int C4 = C >> 2;
    for (; i < n4; i += stride) {
      long long row;
      int c4;
      if (small) {
        const unsigned r = (unsigned)i / (unsigned)C4;
        c4 = (int)((unsigned)i - r * (unsigned)C4);
        row = r;
      } else {
        row = i / C4;
        c4 = (int)(i - row * C4);
      }
      const long long b = small ? (long long)((unsigned)row / (unsigned)P) : row / P;
      const f32x4 k = ((const f32x4*)keep)[b * C4 + c4], v = ((const f32x4*)x)[i];
      ((f32x4*)y)[i] = f32x4{v.x * k.x, v.y * k.y, v.z * k.z, v.w * k.w};
    }
  } else {
    for (; i < n; i += stride) {
      long long row;
      int c;
      if (small) {
        const unsigned r = (unsigned)i / (unsigned)C;
        c = (int)((unsigned)i - r * (unsigned)C);
        row = r;
      } else {
        row = i / C;
        c = (int)(i - row * C);
      }
      const long long b = small ? (long long)((unsigned)row / (unsigned)P) : row / P;
      y[i] = x[i] * keep[b * C + c];
    }
  }
}

}  // namespace

extern "C" int hrnet_burger_mix(const float* u, const float* s, const float* coef_ham, const float* coef_shortcut,
                                float* out, long long rows, int C, hr_stream_t stream) {
  HR_REQUIRE(shape_ok(rows, C), "burger_mix: rows = %lld, C = %d: needs rows >= 1, C a multiple of 16, rows * C <= 2^40",
             rows, C);
  HR_REQUIRE(u && s && coef_ham && coef_shortcut && out, "burger_mix: null pointer (u = %p, s = %p, coef_ham = %p, "
             "coef_shortcut = %p, out = %p)", (const void*)u, (const void*)s, (const void*)coef_ham,
             (const void*)coef_shortcut, (void*)out);
  HR_REQUIRE(out != s, "burger_mix: out aliases s (only u may be overwritten)");
  const long long n = rows * C;
  const bool vec = aligned16(u) && aligned16(s) && aligned16(out);
  const int blocks = blocks_for(n, vec ? 4 : 1, kMixBlocks);
  if (vec) burger_mix_kernel<true><<<blocks, kThreads, 0, (hipStream_t)stream>>>(u, s, coef_ham, coef_shortcut, out, n);
  else burger_mix_kernel<false><<<blocks, kThreads, 0, (hipStream_t)stream>>>(u, s, coef_ham, coef_shortcut, out, n);
  return hr_check_launch("burger_mix");
}

extern "C" int hrnet_burger_mix_scratch(long long rows, int C) {
  if (!shape_ok(rows, C)) return 0;
  return 2 * blocks_for(rows * C, 4, kBwdBlocks);
}

extern "C" int hrnet_burger_mix_bwd(const float* g, const float* out, const float* u, const float* s,
                                    const float* coef_ham, const float* coef_shortcut, float* du, float* ds, float* dcoef,
                                    double* scratch, long long scratch_doubles, long long rows, int C,
                                    hr_stream_t stream) {
  HR_REQUIRE(shape_ok(rows, C), "burger_mix_bwd: rows = %lld, C = %d: needs rows >= 1, C a multiple of 16, rows * C <= "
             "2^40", rows, C);
  HR_REQUIRE(g && out && u && s && coef_ham && coef_shortcut, "burger_mix_bwd: null pointer (g = %p, out = %p, u = %p, "
             "s = %p, coef_ham = %p, coef_shortcut = %p)", (const void*)g, (const void*)out, (const void*)u, (const void*)s,
             (const void*)coef_ham, (const void*)coef_shortcut);
  HR_REQUIRE(du || ds || dcoef, "burger_mix_bwd: du, ds and dcoef are all NULL: nothing to compute");
  HR_REQUIRE(!du || (du != out && du != u && du != s && du != ds), "burger_mix_bwd: du aliases out, u, s or ds (only g "
             "may be overwritten)");
  HR_REQUIRE(!ds || (ds != g && ds != out && ds != u && ds != s), "burger_mix_bwd: ds aliases an input");
  const long long n = rows * C;
  // the grid, and with it the order of every sum, is a function of the shape alone
  const int blocks = blocks_for(n, 4, kBwdBlocks);
  const long long need = dcoef ? 2LL * blocks : 0;
  HR_REQUIRE(need == 0 || (scratch && scratch_doubles >= need), "burger_mix_bwd: scratch of %lld doubles at %p: %lld are "
             "needed (hrnet_burger_mix_scratch)", scratch_doubles, (void*)scratch, need);
  HR_REQUIRE(need == 0 || ((uintptr_t)scratch & 7u) == 0, "burger_mix_bwd: scratch %p is not 8-byte aligned", (void*)scratch);
  const bool vec = aligned16(g) && aligned16(out) && aligned16(u) && aligned16(s) && (!du || aligned16(du)) &&
                   (!ds || aligned16(ds));
  double* partials = dcoef ? scratch : nullptr;
  if (vec) burger_mix_bwd_kernel<true><<<blocks, kThreads, 0, (hipStream_t)stream>>>(g, out, u, s, coef_ham, coef_shortcut,
                                                                                     du, ds, partials, n);
  else burger_mix_bwd_kernel<false><<<blocks, kThreads, 0, (hipStream_t)stream>>>(g, out, u, s, coef_ham, coef_shortcut,
                                                                                  du, ds, partials, n);
  if (const int rc = hr_check_launch("burger_mix_bwd")) return rc;
  if (!dcoef) return HR_OK;
  burger_mix_reduce_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(partials, blocks, dcoef);
  return hr_check_launch("burger_mix_bwd (reduce)");
}

extern "C" int hrnet_dropout2d(const float* x, const float* keep, float* y, int B, long long P, int C, hr_stream_t stream) {
  HR_REQUIRE(B >= 1 && P >= 1 && P <= kMaxElems / B && shape_ok((long long)B * P, C), "dropout2d: B = %d, P = %lld, C = %d: "
             "needs B, P >= 1, C a multiple of 16, B * P * C <= 2^40", B, P, C);
  HR_REQUIRE(x && keep && y, "dropout2d: null pointer (x = %p, keep = %p, y = %p)", (const void*)x, (const void*)keep,
             (void*)y);
  HR_REQUIRE(y != keep, "dropout2d: y aliases keep");
  const long long n = (long long)B * P * C;
  const bool vec = aligned16(x) && aligned16(keep) && aligned16(y);
  const int blocks = blocks_for(n, vec ? 4 : 1, kMixBlocks);
  if (vec) dropout2d_kernel<true><<<blocks, kThreads, 0, (hipStream_t)stream>>>(x, keep, y, n, P, C);
  else dropout2d_kernel<false><<<blocks, kThreads, 0, (hipStream_t)stream>>>(x, keep, y, n, P, C);
  return hr_check_launch("dropout2d");
}
