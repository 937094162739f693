// Multi-view DLT triangulation of tools/evaluate_3D.py (reference lib/models/triangulation_model_utils/multiview.py:
// 120-187; weighting of triangulate_point_from_multiple_views_linear_torch, :142-169). One thread per (sample, joint)
// point: B * K points, a few thousand at most, so the launch is latency-bound and is neither tiled nor put on MFMA.
//
// Per point, every view v with weight w (1 without conf) contributes the two rows w (u P[2] - P[0]) and
// w (v P[2] - P[1]) of the 2V x 4 matrix A, (u, v) in frame pixels (the heat-map point mapped through `to_frame`
// first when it is given). X is the right singular vector of A for its smallest singular value, dehomogenised.
// Everything is float64, and A^T A is never formed (it squares cond(A), ~3e3 on a near-parallel rig):
//   1. the rows are streamed into a 4 x 4 upper-triangular R with Givens rotations (A = Q R, so A and R have the
//      same right singular vectors); A itself is never held;
//   2. a one-sided (Hestenes) Jacobi SVD orthogonalises R's columns, accumulating V, under a fixed sweep cap;
//   3. the column of V whose rotated column of R has the smallest norm is v; X = v[0:3] / v[3] (sign-free).
// Degenerate input: fewer than two views with a nonzero weight gives NaN; v[3] == 0 gives a non-finite X; a
// non-finite input runs into the sweep cap and gives a non-finite X. No input can make the kernel loop or fault.
#include "common.h"

namespace {

constexpr int kTriThreads = 64;
constexpr int kTriMaxViews = 8;
constexpr int kTriSweeps = 16;      // a 4 x 4 converges in 5-7 sweeps at f64 precision
constexpr double kTriEps = 2.220446049250313e-16;   // f64 machine epsilon: a pair this close to orthogonal is done

// one Givens step: rotate row a (entries j..3) into row j of R so that a[j] becomes 0
template <int J>
__device__ __forceinline__ void tri_givens(double (&R)[4][4], double (&a)[4]) {
  const double r = hypot(R[J][J], a[J]);
  if (r == 0.0) return;
  const double c = R[J][J] / r, s = a[J] / r;
#pragma unroll
  for (int k = J; k < 4; ++k) {
    const double rk = R[J][k], ak = a[k];
    R[J][k] = c * rk + s * ak;
    a[k] = c * ak - s * rk;
  }
}

__device__ __forceinline__ void tri_add_row(double (&R)[4][4], double (&a)[4]) {
  tri_givens<0>(R, a);
  tri_givens<1>(R, a);
  tri_givens<2>(R, a);
  tri_givens<3>(R, a);
}

// one Jacobi rotation of columns p < q of W (and V); returns true if it rotated
template <int P, int Q>
__device__ __forceinline__ bool tri_jacobi(double (&W)[4][4], double (&V)[4][4]) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    alpha += W[i][P] * W[i][P];
    beta += W[i][Q] * W[i][Q];
    gamma += W[i][P] * W[i][Q];
  }
  // converged pair (a NaN gamma fails the test and keeps rotating, bounded by the sweep cap)
  if (fabs(gamma) <= kTriEps * sqrt(alpha * beta)) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + hypot(1.0, zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double wp = W[i][P], wq = W[i][Q];
    W[i][P] = c * wp - s * wq;
    W[i][Q] = s * wp + c * wq;
    const double vp = V[i][P], vq = V[i][Q];
    V[i][P] = c * vp - s * vq;
    V[i][Q] = s * vp + c * vq;
  }
  return true;
}

__global__ __launch_bounds__(kTriThreads) void triangulate_kernel(const float* __restrict__ pts,
                                                                  const double* __restrict__ to_frame,
                                                                  const double* __restrict__ proj,
                                                                  const float* __restrict__ conf, float* __restrict__ X,
                                                                  float* __restrict__ pts_frame, int B, int V, int K) {
  const long long t = (long long)blockIdx.x * kTriThreads + threadIdx.x;
  if (t >= (long long)B * K) return;
  const long long b = t / K, k = t - b * K;
  double R[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) R[i][j] = 0.0;
  int weighted = 0;
  for (int v = 0; v < V; ++v) {
    const long long slot = b * V + v;               // b * V + v: the decode kernel's (B*V, K) order
    const long long pi = slot * K + k;
    double u = (double)pts[2 * pi], w = (double)pts[2 * pi + 1];
    if (to_frame) {
      const double* m = to_frame + 6 * slot;
      const double fu = m[0] * u + m[1] * w + m[2];
      w = m[3] * u + m[4] * w + m[5];
      u = fu;
    }
    if (pts_frame) {
      pts_frame[2 * pi] = (float)u;
      pts_frame[2 * pi + 1] = (float)w;
    }
    const double c = conf ? (double)conf[pi] : 1.0;
    if (c != 0.0) ++weighted;                       // a NaN weight counts (and makes X NaN)
    const double* P = proj + 12 * slot;
    double r0[4], r1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r0[j] = c * (u * P[8 + j] - P[j]);
      r1[j] = c * (w * P[8 + j] - P[4 + j]);
    }
    tri_add_row(R, r0);
    tri_add_row(R, r1);
  }
  float* out = X + 3 * t;
  if (weighted < 2) {
    const float nan = __builtin_nanf("");
    out[0] = nan;
    out[1] = nan;
    out[2] = nan;
    return;
  }
  double Vm[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) Vm[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kTriSweeps; ++sweep) {
    bool rotated = tri_jacobi<0, 1>(R, Vm);
    rotated |= tri_jacobi<0, 2>(R, Vm);
    rotated |= tri_jacobi<0, 3>(R, Vm);
    rotated |= tri_jacobi<1, 2>(R, Vm);
    rotated |= tri_jacobi<1, 3>(R, Vm);
    rotated |= tri_jacobi<2, 3>(R, Vm);
    if (!rotated) break;
  }
  // smallest column norm of R V = smallest singular value; selects with compile-time indices keep it in registers
  double n[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) n[j] = R[0][j] * R[0][j] + R[1][j] * R[1][j] + R[2][j] * R[2][j] + R[3][j] * R[3][j];
  double best = n[0], h0 = Vm[0][0], h1 = Vm[1][0], h2 = Vm[2][0], h3 = Vm[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (n[j] < best) {
      best = n[j];
      h0 = Vm[0][j];
      h1 = Vm[1][j];
      h2 = Vm[2][j];
      h3 = Vm[3][j];
    }
  }
  out[0] = (float)(h0 / h3);
  out[1] = (float)(h1 / h3);
  out[2] = (float)(h2 / h3);
}

}  // namespace

extern "C" int hrnet_triangulate(const float* pts, const double* to_frame, const double* proj, const float* conf,
                                 float* X, float* pts_frame, int B, int V, int K, hr_stream_t stream) {
  HR_REQUIRE(pts && proj && X, "triangulate: null argument");
  HR_REQUIRE(V >= 2 && V <= kTriMaxViews, "triangulate: V = %d views (2..%d)", V, kTriMaxViews);
  HR_REQUIRE(B > 0 && K > 0 && (long long)B * V * K <= (1LL << 30), "triangulate: B = %d, V = %d, K = %d", B, V, K);
  const long long n = (long long)B * K;
  const unsigned blocks = (unsigned)((n + kTriThreads - 1) / kTriThreads);
  hipLaunchKernelGGL(triangulate_kernel, dim3(blocks), dim3(kTriThreads), 0, (hipStream_t)stream, pts, to_frame, proj,
                     conf, X, pts_frame, B, V, K);
  return hr_check_launch("triangulate");
}
