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
//
// hrnet_triangulate_ransac (reference lib/utils/misc.py:178-240) chooses the views of each point first - the largest
// set that agrees with a two-view solution, see triangulate_ransac_kernel - and ends with the same DLT over that set.
// Both kernels share the device functions below, called in the same order, so that where the sets coincide the two
// results are the same bits.
//
// hrnet_triangulate_bwd is the gradient of the all-view DLT with respect to the points and the weights, for the 3-D
// training loss (see triangulate_bwd_kernel). It recomputes the forward's SVD from the same inputs with the same
// device functions and needs nothing saved.
#include "common.h"

namespace {

constexpr int kTriThreads = 64;
constexpr int kTriMaxViews = 8;
constexpr int kTriSweeps = 16;      // a 4 x 4 converges in 5-7 sweeps at f64 precision
constexpr double kTriEps = 2.220446049250313e-16;   // f64 machine epsilon: a pair this close to orthogonal is done
constexpr int kRansacGroup = 8;     // lanes per point of the RANSAC kernel (1: one thread per point, 3.3x slower)
constexpr int kRansacMaxHyp = 64;   // all 28 pairs of 8 views, or 64 sampled draws; the key holds 255 - index in 8 bits

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

// frame-pixel point of view `slot` for point index pi: the heat-map point mapped through to_frame when it is given
__device__ __forceinline__ void tri_load_point(const float* __restrict__ pts, const double* __restrict__ to_frame,
                                               long long slot, long long pi, double& u, double& w) {
  u = (double)pts[2 * pi];
  w = (double)pts[2 * pi + 1];
  if (to_frame) {
    const double* m = to_frame + 6 * slot;
    const double fu = m[0] * u + m[1] * w + m[2];
    w = m[3] * u + m[4] * w + m[5];
    u = fu;
  }
}

// the two DLT rows c (u P[2] - P[0]) and c (w P[2] - P[1]) of one view, rotated into R
__device__ __forceinline__ void tri_add_view(double (&R)[4][4], const double* __restrict__ P, double u, double w,
                                             double c) {
  double r0[4], r1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r0[j] = c * (u * P[8 + j] - P[j]);
    r1[j] = c * (w * P[8 + j] - P[4 + j]);
  }
  tri_add_row(R, r0);
  tri_add_row(R, r1);
}

__device__ __forceinline__ void tri_zero(double (&R)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) R[i][j] = 0.0;
}

// Jacobi SVD of R (destroyed); h = the right singular vector of its smallest singular value, not dehomogenised
__device__ __forceinline__ void tri_null_vector(double (&R)[4][4], double (&h)[4]) {
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
  double best = n[0];
  h[0] = Vm[0][0], h[1] = Vm[1][0], h[2] = Vm[2][0], h[3] = Vm[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (n[j] < best) {
      best = n[j];
      h[0] = Vm[0][j];
      h[1] = Vm[1][j];
      h[2] = Vm[2][j];
      h[3] = Vm[3][j];
    }
  }
}

// The SVD of tri_null_vector, step for step, for the backward, which needs all of it: R becomes R V (orthogonal
// columns), Vm holds the right singular vectors and n[j] the SQUARED singular value of column j (the squared norm of
// column j of R V); the columns are not sorted. It is a function of its own so that the forward kernels compile to the
// code they had before the backward existed.
__device__ __forceinline__ void tri_svd(double (&R)[4][4], double (&Vm)[4][4], double (&n)[4]) {
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
#pragma unroll
  for (int j = 0; j < 4; ++j) n[j] = R[0][j] * R[0][j] + R[1][j] * R[1][j] + R[2][j] * R[2][j] + R[3][j] * R[3][j];
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
  tri_zero(R);
  int weighted = 0;
  for (int v = 0; v < V; ++v) {
    const long long slot = b * V + v;               // b * V + v: the decode kernel's (B*V, K) order
    const long long pi = slot * K + k;
    double u, w;
    tri_load_point(pts, to_frame, slot, pi, u, w);
    if (pts_frame) {
      pts_frame[2 * pi] = (float)u;
      pts_frame[2 * pi + 1] = (float)w;
    }
    const double c = conf ? (double)conf[pi] : 1.0;
    if (c != 0.0) ++weighted;                       // a NaN weight counts (and makes X NaN)
    tri_add_view(R, proj + 12 * slot, u, w, c);
  }
  float* out = X + 3 * t;
  if (weighted < 2) {
    const float nan = __builtin_nanf("");
    out[0] = nan;
    out[1] = nan;
    out[2] = nan;
    return;
  }
  double h[4];
  tri_null_vector(R, h);
  out[0] = (float)(h[0] / h[3]);
  out[1] = (float)(h[1] / h[3]);
  out[2] = (float)(h[2] / h[3]);
}

// Backward of triangulate_kernel, one thread per point, for the 3-D training loss (the reference back-propagates
// through torch.svd, lib/models/triangulation_model_utils/multiview.py:164). Nothing is saved by the forward: R and its
// Jacobi SVD are recomputed from the inputs with the forward's device functions in the forward's order, so h is the
// forward's h, and the SVD already holds what the derivative needs - all four right singular vectors v_j (columns of
// Vm) and squared singular values n_j. With m the forward's column (h = v_m) and g = dL/dX:
//   g^ = dL/dh = [g / h3, -(g . h[0:3]) / h3^2]
//   z  = -sum_{j != m} v_j (v_j . g^) / (n_j - n_m)            (first-order perturbation of a singular vector)
//   dL/dA = (A z) h^T + (A h) z^T; row 2v of A is c a0 with a0 = u P[2] - P[0] (a1 = w P[2] - P[1] for row 2v+1), so
//   dL/du = c^2 ((a0 . z)(h . P[2]) + (a0 . h)(z . P[2])), dL/dw likewise with a1,
//   dL/dc = 2 c ((a0 . z)(a0 . h) + (a1 . z)(a1 . h)),
// and (dL/du, dL/dw) goes back through the 2 x 2 part of to_frame to the given points. A^T A is never formed. The sign
// of h cancels. A view of weight 0 gets exact zeros (c^2 and c are factors). A point with fewer than two weighted views
// gets NaN in every view, as its X is NaN; a non-finite input makes the point's gradients NaN through the arithmetic.
// A vanishing n_j - n_m gives what the formula gives (huge or non-finite), as torch.svd's backward does. The index m
// is only compared against compile-time column numbers, so Vm and n stay in registers.
__global__ __launch_bounds__(kTriThreads) void triangulate_bwd_kernel(
    const float* __restrict__ pts, const double* __restrict__ to_frame, const double* __restrict__ proj,
    const float* __restrict__ conf, const float* __restrict__ gX, float* __restrict__ dpts, float* __restrict__ dconf,
    int B, int V, int K) {
  const long long t = (long long)blockIdx.x * kTriThreads + threadIdx.x;
  if (t >= (long long)B * K) return;
  const long long b = t / K, k = t - b * K;
  double R[4][4];
  tri_zero(R);
  int weighted = 0;
  for (int v = 0; v < V; ++v) {
    const long long slot = b * V + v;
    const long long pi = slot * K + k;
    double u, w;
    tri_load_point(pts, to_frame, slot, pi, u, w);
    const double c = conf ? (double)conf[pi] : 1.0;
    if (c != 0.0) ++weighted;
    tri_add_view(R, proj + 12 * slot, u, w, c);
  }
  if (weighted < 2) {
    const float nan = __builtin_nanf("");
    for (int v = 0; v < V; ++v) {
      const long long pi = (b * V + v) * K + k;
      dpts[2 * pi] = nan;
      dpts[2 * pi + 1] = nan;
      if (dconf) dconf[pi] = nan;
    }
    return;
  }
  double Vm[4][4], n[4];
  tri_svd(R, Vm, n);
  // the forward's choice: the first column of smallest norm
  double best = n[0];
  int m = 0;
  double h[4] = {Vm[0][0], Vm[1][0], Vm[2][0], Vm[3][0]};
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (n[j] < best) {
      best = n[j];
      m = j;
      h[0] = Vm[0][j];
      h[1] = Vm[1][j];
      h[2] = Vm[2][j];
      h[3] = Vm[3][j];
    }
  }
  const double g0 = (double)gX[3 * t], g1 = (double)gX[3 * t + 1], g2 = (double)gX[3 * t + 2];
  const double gh[4] = {g0 / h[3], g1 / h[3], g2 / h[3], -(g0 * h[0] + g1 * h[1] + g2 * h[2]) / (h[3] * h[3])};
  double z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double dot = Vm[0][j] * gh[0] + Vm[1][j] * gh[1] + Vm[2][j] * gh[2] + Vm[3][j] * gh[3];
    const double wgt = j == m ? 0.0 : -dot / (n[j] - best);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] += wgt * Vm[i][j];
  }
  for (int v = 0; v < V; ++v) {
    const long long slot = b * V + v;
    const long long pi = slot * K + k;
    double u, w;
    tri_load_point(pts, to_frame, slot, pi, u, w);
    const double c = conf ? (double)conf[pi] : 1.0;
    const double* P = proj + 12 * slot;
    double a0z = 0.0, a0h = 0.0, a1z = 0.0, a1h = 0.0, p2z = 0.0, p2h = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double a0 = u * P[8 + j] - P[j], a1 = w * P[8 + j] - P[4 + j];
      a0z += a0 * z[j];
      a0h += a0 * h[j];
      a1z += a1 * z[j];
      a1h += a1 * h[j];
      p2z += P[8 + j] * z[j];
      p2h += P[8 + j] * h[j];
    }
    const double du = c * c * (a0z * p2h + a0h * p2z), dw = c * c * (a1z * p2h + a1h * p2z);
    double dx = du, dy = dw;
    if (to_frame) {
      const double* mt = to_frame + 6 * slot;
      dx = mt[0] * du + mt[3] * dw;
      dy = mt[1] * du + mt[4] * dw;
    }
    dpts[2 * pi] = (float)dx;
    dpts[2 * pi + 1] = (float)dy;
    if (dconf) dconf[pi] = (float)(2.0 * c * (a0z * a0h + a1z * a1h));
  }
}

// RANSAC over the views (reference lib/utils/misc.py:178-240 with direct_optimization off). A group of kRansacGroup
// adjacent lanes works on one point, so a wave holds 64 / kRansacGroup points:
//   1. lane g of the group takes hypotheses g, g + kRansacGroup, ... of the point's table in ascending order. For a
//      pair (i, j) it solves the two-view DLT of views i and j (i first), reprojects X into every view and collects
//      {i, j} with every view whose error - HALF the pixel distance, the reference's unit - is below epsilon. It keeps
//      its own largest set, the earlier one on a tie;
//   2. an integer max over the group (xor shuffles inside the group) of the key [set size | 255 - hypothesis index |
//      view mask] picks the largest set and, among equals, the first in table order - the reference's `>` rule;
//   3. every lane of the group solves the DLT over that set, views ascending, with the device functions and the row
//      order of triangulate_kernel; lane 0 writes X and the mask, lanes 0..V-1 the frame points.
// The result does not depend on kRansacGroup: the key orders hypotheses by table index whichever lane solved them.
// A pair with i == j or an index outside 0..V-1 is skipped; with no usable pair the set is every view. A non-finite
// point or projection matrix in any view of a point makes its X NaN. Every loop is bounded by n_hyp, V or the sweep
// cap.
template <int G>
__global__ __launch_bounds__(kTriThreads) void triangulate_ransac_kernel(
    const float* __restrict__ pts, const double* __restrict__ to_frame, const double* __restrict__ proj,
    const int* __restrict__ pairs, int n_hyp, int per_point, double epsilon, float* __restrict__ X,
    int* __restrict__ inliers, float* __restrict__ pts_frame, int B, int V, int K) {
  static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && kTriThreads % G == 0, "lane group: a power of two");
  const long long t = ((long long)blockIdx.x * kTriThreads + threadIdx.x) / G;   // point; a group leaves together
  const int g = threadIdx.x % G;
  if (t >= (long long)B * K) return;
  const long long b = t / K, k = t - b * K;
  const int* table = pairs + (per_point ? 2 * t * n_hyp : 0);
  double R[4][4], h[4];
  unsigned best = 0u;
  for (int hyp = g; hyp < n_hyp; hyp += G) {
    const int i = table[2 * hyp], j = table[2 * hyp + 1];
    if (i == j || (unsigned)i >= (unsigned)V || (unsigned)j >= (unsigned)V) continue;
    tri_zero(R);
    double u, w;
    tri_load_point(pts, to_frame, b * V + i, (b * V + i) * K + k, u, w);
    tri_add_view(R, proj + 12 * (b * V + i), u, w, 1.0);
    tri_load_point(pts, to_frame, b * V + j, (b * V + j) * K + k, u, w);
    tri_add_view(R, proj + 12 * (b * V + j), u, w, 1.0);
    tri_null_vector(R, h);
    const double x = h[0] / h[3], y = h[1] / h[3], z = h[2] / h[3];
    unsigned mask = (1u << i) | (1u << j);
    for (int v = 0; v < V; ++v) {
      const long long slot = b * V + v;
      tri_load_point(pts, to_frame, slot, slot * K + k, u, w);
      const double* P = proj + 12 * slot;
      const double pz = P[8] * x + P[9] * y + P[10] * z + P[11];
      const double du = u - (P[0] * x + P[1] * y + P[2] * z + P[3]) / pz;
      const double dw = w - (P[4] * x + P[5] * y + P[6] * z + P[7]) / pz;
      if (0.5 * sqrt(du * du + dw * dw) < epsilon) mask |= 1u << v;      // a NaN error keeps the view out
    }
    const unsigned key = ((unsigned)__popc(mask) << 16) | ((unsigned)(255 - hyp) << 8) | mask;
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)best, o, G);
    best = other > best ? other : best;
  }
  const unsigned set = best ? (best & 0xffu) : ((1u << V) - 1u);
  tri_zero(R);
  double poison = 0.0;                               // 0 * x summed over the point's inputs: NaN if one is not finite
  for (int v = 0; v < V; ++v) {
    const long long slot = b * V + v;
    const long long pi = slot * K + k;
    double u, w;
    tri_load_point(pts, to_frame, slot, pi, u, w);
    if (pts_frame && g == v % G) {
      pts_frame[2 * pi] = (float)u;
      pts_frame[2 * pi + 1] = (float)w;
    }
    poison += 0.0 * u + 0.0 * w;
#pragma unroll
    for (int j = 0; j < 12; ++j) poison += 0.0 * proj[12 * slot + j];
    if (set >> v & 1u) tri_add_view(R, proj + 12 * slot, u, w, 1.0);
  }
  tri_null_vector(R, h);
  if (g == 0) {
    // a view with a non-finite point never passes the threshold, so the rule alone would drop it and hide the fault
    // upstream; as in triangulate_kernel, a non-finite input of any view makes the point's X non-finite (NaN here)
    float* out = X + 3 * t;
    const bool finite = poison == 0.0;
    const float nan = __builtin_nanf("");
    out[0] = finite ? (float)(h[0] / h[3]) : nan;
    out[1] = finite ? (float)(h[1] / h[3]) : nan;
    out[2] = finite ? (float)(h[2] / h[3]) : nan;
    inliers[t] = (int)set;
  }
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

extern "C" int hrnet_triangulate_bwd(const float* pts, const double* to_frame, const double* proj, const float* conf,
                                     const float* gX, float* dpts, float* dconf, int B, int V, int K,
                                     hr_stream_t stream) {
  HR_REQUIRE(pts && proj && gX && dpts, "triangulate_bwd: null argument");
  HR_REQUIRE(V >= 2 && V <= kTriMaxViews, "triangulate_bwd: V = %d views (2..%d)", V, kTriMaxViews);
  HR_REQUIRE(B > 0 && K > 0 && (long long)B * V * K <= (1LL << 30), "triangulate_bwd: B = %d, V = %d, K = %d", B, V,
             K);
  const long long n = (long long)B * K;
  const unsigned blocks = (unsigned)((n + kTriThreads - 1) / kTriThreads);
  hipLaunchKernelGGL(triangulate_bwd_kernel, dim3(blocks), dim3(kTriThreads), 0, (hipStream_t)stream, pts, to_frame,
                     proj, conf, gX, dpts, dconf, B, V, K);
  return hr_check_launch("triangulate_bwd");
}

extern "C" int hrnet_triangulate_ransac(const float* pts, const double* to_frame, const double* proj, const int* pairs,
                                        int n_hyp, int pairs_per_point, double epsilon, float* X, int* inliers,
                                        float* pts_frame, int B, int V, int K, hr_stream_t stream) {
  HR_REQUIRE(pts && proj && X && inliers, "triangulate_ransac: null argument");
  HR_REQUIRE(V >= 2 && V <= kTriMaxViews, "triangulate_ransac: V = %d views (2..%d)", V, kTriMaxViews);
  HR_REQUIRE(B > 0 && K > 0 && (long long)B * V * K <= (1LL << 30), "triangulate_ransac: B = %d, V = %d, K = %d", B, V,
             K);
  HR_REQUIRE(n_hyp >= 0 && n_hyp <= kRansacMaxHyp, "triangulate_ransac: n_hyp = %d hypotheses (0..%d)", n_hyp,
             kRansacMaxHyp);
  HR_REQUIRE(pairs || n_hyp == 0, "triangulate_ransac: null pair table with n_hyp = %d", n_hyp);
  HR_REQUIRE(!(epsilon != epsilon), "triangulate_ransac: epsilon is NaN");
  const long long n = (long long)B * K * kRansacGroup;
  const unsigned blocks = (unsigned)((n + kTriThreads - 1) / kTriThreads);
  hipLaunchKernelGGL(triangulate_ransac_kernel<kRansacGroup>, dim3(blocks), dim3(kTriThreads), 0, (hipStream_t)stream,
                     pts, to_frame, proj, pairs, n_hyp, pairs_per_point, epsilon, X, inliers, pts_frame, B, V, K);
  return hr_check_launch("triangulate_ransac");
}
