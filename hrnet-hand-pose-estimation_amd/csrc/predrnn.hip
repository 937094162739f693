// The spatio-temporal LSTM cell of PredRNN (reference lib/models/predrnn.py:7-58) between its convolutions, and the
// MaxPool2d(2, 2) of the model's ResNet tail (include/hrnet_hip.h: hrnet_sample_stats, hrnet_stlstm_gates,
// hrnet_stlstm_out, hrnet_maxpool2d_2x2). f32 NHWC, inference.
//
// A cell runs five convolutions (hipnet.conv_kxk); four of them end in nn.LayerNorm([C, W, W]): a normalisation over ALL
// C H W elements of a sample with a per-element affine of that shape. Around them the reference splits, adds and gates
// in about thirty element-wise ops. Here that is
//
//   hrnet_sample_stats   (mean, rstd) of every sample of the raw conv_x, conv_h and conv_m outputs, one entry for all three
//   hrnet_stlstm_gates   LayerNorm of the three maps applied on load, the six gates, c_new and m_new written into the two
//                        halves of the layer's memory map (so torch.cat((c_new, m_new)) is never a copy), and
//                        o_pre = LN(xc)[o_x] + LN(hc)[o_h]
//   hrnet_sample_stats   of the raw conv_o output
//   hrnet_stlstm_out     h_new = sigmoid(o_pre + LN(oc)) * tanh(conv_last(mem))
//
// and no normalised tensor ever reaches memory. o_pre is WRITTEN by the gates kernel (one float4 out, one in) and not
// recomputed by the out kernel, which would read two activations and four affine values per float4 again.
//
// Statistics. Two kernels per entry, no atomics, no in-launch hand-off between workgroups (csrc/predrnn_plan.h states the
// partition): the first gives every part of PRS_CHUNK elements to one workgroup, the second adds a sample's parts. All
// sums are double. The data is shifted by the sample's first element K before it is squared,
//   S1 = sum (x - K), S2 = sum (x - K)^2, mean = K + S1 / n, var = (S2 - S1^2 / n) / n  (>= 0), rstd = 1 / sqrt(var + eps),
// which is the variance of the shifted data: the cancellation in S2 - S1^2 / n is that of data whose mean is (mean - K),
// a few sigma at the most, and not that of E[x^2] - mean^2 at the data's own mean; x - K is exact in double for float x.
// A constant map gives S1 = S2 = 0 and rstd = 1 / sqrt(eps) exactly. mean and rstd are rounded to float once.
// Order of the sums, fixed by the shape: a thread adds its PRS_VEC float4 in load order, x y z w; a wave adds its lanes by
// the shuffle tree 32, 16, 8, 4, 2, 1; thread 0 adds the four waves 0 .. 3; the second kernel's lane l adds parts
// l, l + 64, ... and the same tree closes it.
//
// Gates. One thread owns four consecutive channels c .. c + 3 (< nh) of one pixel: it reads the 14 float4 of the three
// raw maps, their 28 affine float4 (the LayerNorm weights repacked once to (H, W, C), so they are read along the channel
// axis like the maps), its own float4 of c_t and of m_t, and only then writes. c_t and m_t may therefore be the very
// slices of `mem` that c_new and m_new go to (the layer's own map from the previous time step): no thread reads what
// another writes. The arithmetic is the reference's, in its order:
//   LN(v) = fma((v - mean) * rstd, weight, bias)
//   i = sigmoid(i_x + i_h), f = sigmoid(f_x + f_h + 1), g = tanh(g_x + g_h), c_new = f * c_t + i * g
//   i' = sigmoid(i'_x + i_m), f' = sigmoid(f'_x + f_m + 1), g' = tanh(g'_x + g_m), m_new = f' * m_t + i' * g'
// with sigmoid(v) = 1 / (1 + expf(-v)) and tanhf. The channel slices of xc are i f g i' f' g' o, of hc i f g o, of mc i f g.
#include "common.h"
#include "predrnn_plan.h"

#define PRG_THREADS 256

struct PrsArgs {
  const float* x[PRS_MAPS];
  PrsPlan p;
};

__device__ __forceinline__ double prs_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(PRS_THREADS) void prs_part_kernel(PrsArgs a, double* __restrict__ scratch) {
  __shared__ double red[2][PRS_THREADS / 64];
  const long long blk = blockIdx.x;
  int m = 0;
#pragma unroll
  for (int i = 1; i < PRS_MAPS; ++i)
    if (i < a.p.maps && blk >= a.p.first[i]) m = i;
  const long long local = blk - a.p.first[m];
  const int parts = a.p.parts[m];
  const long long b = local / parts;
  const long long part = local - b * parts;
  const long long n = a.p.n[m];
  const float* x = a.x[m] + (size_t)b * n;
  const double K = (double)x[0];
  const long long e0 = part * PRS_CHUNK;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int i = 0; i < PRS_VEC; ++i) {
    const long long e = e0 + ((long long)i * PRS_THREADS + threadIdx.x) * 4;
    if (e < n) {
      const float4 v = *reinterpret_cast<const float4*>(x + e);
      const double d0 = (double)v.x - K, d1 = (double)v.y - K, d2 = (double)v.z - K, d3 = (double)v.w - K;
      s += d0; q = fma(d0, d0, q);
      s += d1; q = fma(d1, d1, q);
      s += d2; q = fma(d2, d2, q);
      s += d3; q = fma(d3, d3, q);
    }
  }
  s = prs_wave_sum(s);
  q = prs_wave_sum(q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = s; red[1][wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = red[0][0], tq = red[1][0];
#pragma unroll
    for (int w = 1; w < PRS_THREADS / 64; ++w) { ts += red[0][w]; tq += red[1][w]; }
    scratch[2 * blk] = ts;
    scratch[2 * blk + 1] = tq;
  }
}

// one wave per (map, sample): stats[(m B + b) 2] = mean, [.. + 1] = rstd
__global__ __launch_bounds__(64) void prs_finish_kernel(PrsArgs a, const double* __restrict__ scratch, float* __restrict__ stats,
                                                        double eps) {
  const int m = blockIdx.x / a.p.B, b = blockIdx.x - m * a.p.B;
  const int parts = a.p.parts[m];
  const long long n = a.p.n[m];
  const double* part = scratch + 2 * (a.p.first[m] + (long long)b * parts);
  double s = 0.0, q = 0.0;
  for (int k = threadIdx.x; k < parts; k += 64) { s += part[2 * k]; q += part[2 * k + 1]; }
  s = prs_wave_sum(s);
  q = prs_wave_sum(q);
  if (threadIdx.x == 0) {
    const double K = (double)a.x[m][(size_t)b * n];
    const double dn = (double)n;
    const double mean = K + s / dn;
    double var = (q - s * s / dn) / dn;
    var = var > 0.0 ? var : 0.0;
    stats[2 * blockIdx.x] = (float)mean;
    stats[2 * blockIdx.x + 1] = (float)(1.0 / sqrt(var + eps));
  }
}

// ---------------------------------------------------------------------------------------------------------- gates
struct PrgArgs {
  const float *xc, *hc, *mc, *stats;
  const float *wx, *bx, *wh, *bh, *wm, *bm;
  const float *c_t, *m_t;
  float *mem, *o_pre;
  int ldc, c_off, ldmt, m_off, ldmem;
  int B, nh, q;             // q = nh / 4
  long long HW, total;      // total = B HW q threads with work
};

__device__ __forceinline__ float4 prg_ld(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float4 prg_ln(const float* x, const float* w, const float* b, float mean, float rstd) {
  const float4 v = prg_ld(x), g = prg_ld(w), o = prg_ld(b);
  float4 r;
  r.x = fmaf((v.x - mean) * rstd, g.x, o.x);
  r.y = fmaf((v.y - mean) * rstd, g.y, o.y);
  r.z = fmaf((v.z - mean) * rstd, g.z, o.z);
  r.w = fmaf((v.w - mean) * rstd, g.w, o.w);
  return r;
}

__device__ __forceinline__ float prg_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// f * s + i * g of one lane, the reference's order: sigmoid(a_i + b_i), sigmoid(a_f + b_f + 1), tanh(a_g + b_g)
__device__ __forceinline__ float prg_state(float ai, float bi, float af, float bf, float ag, float bg, float s) {
  const float i = prg_sigmoid(ai + bi);
  const float f = prg_sigmoid(af + bf + 1.0f);
  const float g = tanhf(ag + bg);
  return f * s + i * g;
}

__device__ __forceinline__ float4 prg_state4(float4 ai, float4 bi, float4 af, float4 bf, float4 ag, float4 bg, float4 s) {
  float4 r;
  r.x = prg_state(ai.x, bi.x, af.x, bf.x, ag.x, bg.x, s.x);
  r.y = prg_state(ai.y, bi.y, af.y, bf.y, ag.y, bg.y, s.y);
  r.z = prg_state(ai.z, bi.z, af.z, bf.z, ag.z, bg.z, s.z);
  r.w = prg_state(ai.w, bi.w, af.w, bf.w, ag.w, bg.w, s.w);
  return r;
}

// no __restrict__: c_t and m_t may be slices of mem
__global__ __launch_bounds__(PRG_THREADS) void prg_gates_kernel(PrgArgs a) {
  const long long u = (long long)blockIdx.x * PRG_THREADS + threadIdx.x;
  if (u >= a.total) return;
  const int c = (int)(u % a.q) * 4;
  const long long bp = u / a.q;          // pixel of the batch
  const long long b = bp / a.HW;
  const long long p = bp - b * a.HW;     // pixel of the sample: the affine's row
  const int nh = a.nh;
  const float mx = a.stats[2 * b], rx = a.stats[2 * b + 1];
  const float mh = a.stats[2 * (a.B + b)], rh = a.stats[2 * (a.B + b) + 1];
  const float mm = a.stats[2 * (2 * a.B + b)], rm = a.stats[2 * (2 * a.B + b) + 1];
  const float* x = a.xc + (size_t)bp * 7 * nh + c;
  const float* wx = a.wx + (size_t)p * 7 * nh + c;
  const float* bx = a.bx + (size_t)p * 7 * nh + c;
  const float* h = a.hc + (size_t)bp * 4 * nh + c;
  const float* wh = a.wh + (size_t)p * 4 * nh + c;
  const float* bh = a.bh + (size_t)p * 4 * nh + c;
  const float* mc = a.mc + (size_t)bp * 3 * nh + c;
  const float* wm = a.wm + (size_t)p * 3 * nh + c;
  const float* bm = a.bm + (size_t)p * 3 * nh + c;
  const float4 ct = prg_ld(a.c_t + (size_t)bp * a.ldc + a.c_off + c);
  const float4 mt = prg_ld(a.m_t + (size_t)bp * a.ldmt + a.m_off + c);
  const float4 cn = prg_state4(prg_ln(x, wx, bx, mx, rx), prg_ln(h, wh, bh, mh, rh),
                               prg_ln(x + nh, wx + nh, bx + nh, mx, rx), prg_ln(h + nh, wh + nh, bh + nh, mh, rh),
                               prg_ln(x + 2 * nh, wx + 2 * nh, bx + 2 * nh, mx, rx),
                               prg_ln(h + 2 * nh, wh + 2 * nh, bh + 2 * nh, mh, rh), ct);
  const float4 mn = prg_state4(prg_ln(x + 3 * nh, wx + 3 * nh, bx + 3 * nh, mx, rx), prg_ln(mc, wm, bm, mm, rm),
                               prg_ln(x + 4 * nh, wx + 4 * nh, bx + 4 * nh, mx, rx),
                               prg_ln(mc + nh, wm + nh, bm + nh, mm, rm),
                               prg_ln(x + 5 * nh, wx + 5 * nh, bx + 5 * nh, mx, rx),
                               prg_ln(mc + 2 * nh, wm + 2 * nh, bm + 2 * nh, mm, rm), mt);
  const float4 ox = prg_ln(x + 6 * nh, wx + 6 * nh, bx + 6 * nh, mx, rx);
  const float4 oh = prg_ln(h + 3 * nh, wh + 3 * nh, bh + 3 * nh, mh, rh);
  float4 op;
  op.x = ox.x + oh.x; op.y = ox.y + oh.y; op.z = ox.z + oh.z; op.w = ox.w + oh.w;
  float* o = a.mem + (size_t)bp * a.ldmem + c;
  *reinterpret_cast<float4*>(o) = cn;
  *reinterpret_cast<float4*>(o + nh) = mn;
  *reinterpret_cast<float4*>(a.o_pre + (size_t)bp * nh + c) = op;
}

struct ProArgs {
  const float *oc, *stats, *wo, *bo, *o_pre, *last;
  float* h_new;
  int nh, q;
  long long HW, total;
};

__global__ __launch_bounds__(PRG_THREADS) void prg_out_kernel(ProArgs a) {
  const long long u = (long long)blockIdx.x * PRG_THREADS + threadIdx.x;
  if (u >= a.total) return;
  const int c = (int)(u % a.q) * 4;
  const long long bp = u / a.q;
  const long long b = bp / a.HW;
  const long long p = bp - b * a.HW;
  const size_t at = (size_t)bp * a.nh + c, row = (size_t)p * a.nh + c;
  const float4 o = prg_ln(a.oc + at, a.wo + row, a.bo + row, a.stats[2 * b], a.stats[2 * b + 1]);
  const float4 pre = prg_ld(a.o_pre + at), l = prg_ld(a.last + at);
  float4 r;
  r.x = prg_sigmoid(pre.x + o.x) * tanhf(l.x);
  r.y = prg_sigmoid(pre.y + o.y) * tanhf(l.y);
  r.z = prg_sigmoid(pre.z + o.z) * tanhf(l.z);
  r.w = prg_sigmoid(pre.w + o.w) * tanhf(l.w);
  *reinterpret_cast<float4*>(a.h_new + at) = r;
}

// ----------------------------------------------------------------------------------------------------------- pool
struct PrpArgs {
  const float* x;
  float* y;
  int H, W, Ho, Wo, q, ldx, x_off, ldy, y_off;
  long long total;          // N Ho Wo q
};

// torch's rule: a NaN wins
__device__ __forceinline__ float prp_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(PRG_THREADS) void prp_pool_kernel(PrpArgs a) {
  const long long u = (long long)blockIdx.x * PRG_THREADS + threadIdx.x;
  if (u >= a.total) return;
  const int c = (int)(u % a.q) * 4;
  long long t = u / a.q;
  const int wo = (int)(t % a.Wo);
  t /= a.Wo;
  const int ho = (int)(t % a.Ho);
  const long long n = t / a.Ho;
  const float* r0 = a.x + (((size_t)n * a.H + 2 * ho) * a.W + 2 * wo) * a.ldx + a.x_off + c;
  const float* r1 = r0 + (size_t)a.W * a.ldx;
  const float4 v00 = prg_ld(r0), v01 = prg_ld(r0 + a.ldx), v10 = prg_ld(r1), v11 = prg_ld(r1 + a.ldx);
  float4 r;
  r.x = prp_max(prp_max(prp_max(v00.x, v01.x), v10.x), v11.x);
  r.y = prp_max(prp_max(prp_max(v00.y, v01.y), v10.y), v11.y);
  r.z = prp_max(prp_max(prp_max(v00.z, v01.z), v10.z), v11.z);
  r.w = prp_max(prp_max(prp_max(v00.w, v01.w), v10.w), v11.w);
  *reinterpret_cast<float4*>(a.y + (((size_t)n * a.Ho + ho) * a.Wo + wo) * a.ldy + a.y_off + c) = r;
}

// ---------------------------------------------------------------------------------------------------------- entries
static bool pr_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// do the byte ranges [a, a + na floats) and [b, b + nb floats) meet?
static bool pr_overlap(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

extern "C" int hrnet_sample_stats_scratch(int B, long long n0, long long n1, long long n2, long long* bytes) {
  HR_REQUIRE(bytes, "sample_stats_scratch: null bytes");
  const long long n[PRS_MAPS] = {n0, n1, n2};
  PrsPlan p;
  HR_REQUIRE(prs_plan(B, n, &p), "sample_stats_scratch: B = %d, n = %lld, %lld, %lld: needs B >= 1, sizes that are "
             "multiples of 4 with the maps present first, and at most 2^31 - 1 parts of %d elements", B, n0, n1, n2, PRS_CHUNK);
  *bytes = p.bytes;
  return HR_OK;
}

extern "C" int hrnet_sample_stats(const float* x0, const float* x1, const float* x2, long long n0, long long n1, long long n2,
                                  int B, double eps, void* scratch, long long scratch_bytes, float* stats, hr_stream_t stream) {
  PrsArgs a;
  const long long n[PRS_MAPS] = {n0, n1, n2};
  HR_REQUIRE(prs_plan(B, n, &a.p), "sample_stats: B = %d, n = %lld, %lld, %lld: needs B >= 1, sizes that are multiples of 4 "
             "with the maps present first, and at most 2^31 - 1 parts of %d elements", B, n0, n1, n2, PRS_CHUNK);
  a.x[0] = x0; a.x[1] = x1; a.x[2] = x2;
  for (int m = 0; m < PRS_MAPS; ++m) {
    HR_REQUIRE((a.x[m] != nullptr) == (n[m] != 0), "sample_stats: map %d: a pointer and a size go together", m);
    HR_REQUIRE(pr_aligned16(a.x[m]), "sample_stats: map %d must be 16-byte aligned", m);
  }
  HR_REQUIRE(scratch && stats, "sample_stats: null scratch or stats");
  HR_REQUIRE(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)stats & 3) == 0, "sample_stats: scratch must be 8-byte and stats "
             "4-byte aligned");
  HR_REQUIRE(scratch_bytes >= a.p.bytes, "sample_stats: scratch of %lld bytes, %lld needed", scratch_bytes, a.p.bytes);
  HR_REQUIRE(eps >= 0.0, "sample_stats: eps = %g", eps);
  hipLaunchKernelGGL(prs_part_kernel, dim3((unsigned)a.p.blocks), dim3(PRS_THREADS), 0, (hipStream_t)stream, a,
                     (double*)scratch);
  hipLaunchKernelGGL(prs_finish_kernel, dim3((unsigned)(a.p.maps * B)), dim3(64), 0, (hipStream_t)stream, a,
                     (const double*)scratch, stats, eps);
  return hr_check_launch("sample_stats");
}

// B H W nh / 4 threads in a grid: 0 if the shape cannot be served
static int prg_shape(const char* what, int B, int H, int W, int nh, long long* HW, long long* total) {
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && nh >= 4 && nh % 4 == 0, "%s: B = %d, H = %d, W = %d, nh = %d: needs all >= 1 and nh "
             "a multiple of 4", what, B, H, W, nh);
  *HW = (long long)H * W;
  HR_REQUIRE(*HW <= 0x7fffffffLL / B && *HW * B <= (0x7fffffffLL * (PRG_THREADS / 2)) / nh, "%s: B = %d maps of %d x %d x %d: "
             "too many elements for one launch", what, B, H, W, nh);
  *total = *HW * B * (nh / 4);
  return HR_OK;
}

extern "C" int hrnet_stlstm_gates(const float* xc, const float* hc, const float* mc, const float* stats, const float* wx,
                                  const float* bx, const float* wh, const float* bh, const float* wm, const float* bm,
                                  const float* c_t, int ldc, int c_off, const float* m_t, int ldmt, int m_off, float* mem,
                                  int ldmem, float* o_pre, int B, int H, int W, int nh, hr_stream_t stream) {
  PrgArgs a;
  HR_REQUIRE(xc && hc && mc && stats && wx && bx && wh && bh && wm && bm && c_t && m_t && mem && o_pre,
             "stlstm_gates: null argument");
  int rc = prg_shape("stlstm_gates", B, H, W, nh, &a.HW, &a.total);
  if (rc) return rc;
  HR_REQUIRE(ldc % 4 == 0 && c_off % 4 == 0 && c_off >= 0 && (long long)c_off + nh <= ldc, "stlstm_gates: c_t channels [%d, %d "
             "+ %d) in a row of %d: needs multiples of 4 and a slice inside the row", c_off, c_off, nh, ldc);
  HR_REQUIRE(ldmt % 4 == 0 && m_off % 4 == 0 && m_off >= 0 && (long long)m_off + nh <= ldmt, "stlstm_gates: m_t channels [%d, "
             "%d + %d) in a row of %d: needs multiples of 4 and a slice inside the row", m_off, m_off, nh, ldmt);
  HR_REQUIRE(ldmem % 4 == 0 && 2LL * nh <= ldmem, "stlstm_gates: ldmem = %d: needs a multiple of 4 that holds 2 nh = %d", ldmem,
             2 * nh);
  const long long pix = a.HW * B;
  HR_REQUIRE(pix <= 0x7fffffffffffLL / ldc && pix <= 0x7fffffffffffLL / ldmt && pix <= 0x7fffffffffffLL / ldmem,
             "stlstm_gates: a row length is too large for %lld pixels", pix);
  const void* al[] = {xc, hc, mc, wx, bx, wh, bh, wm, bm, c_t, m_t, mem, o_pre};
  for (const void* p : al) HR_REQUIRE(pr_aligned16(p), "stlstm_gates: every map must be 16-byte aligned");
  // the states may be the slices of mem that are written, element for element, and overlap it in no other way
  const long long nmem = pix * ldmem;
  if (pr_overlap(c_t, pix * ldc, mem, nmem))
    HR_REQUIRE(c_t == mem && ldc == ldmem && c_off == 0, "stlstm_gates: c_t overlaps mem but is not its slice [0, nh) (same "
               "pointer and row length, c_off 0)");
  if (pr_overlap(m_t, pix * ldmt, mem, nmem))
    HR_REQUIRE(m_t == mem && ldmt == ldmem && m_off == nh, "stlstm_gates: m_t overlaps mem but is not its slice [nh, 2 nh) "
               "(same pointer and row length, m_off nh)");
  const struct { const void* p; long long n; } in[] = {
      {xc, pix * 7 * nh}, {hc, pix * 4 * nh}, {mc, pix * 3 * nh}, {stats, 6LL * B}, {wx, a.HW * 7 * nh}, {bx, a.HW * 7 * nh},
      {wh, a.HW * 4 * nh}, {bh, a.HW * 4 * nh}, {wm, a.HW * 3 * nh}, {bm, a.HW * 3 * nh}};
  for (const auto& r : in)
    HR_REQUIRE(!pr_overlap(r.p, r.n, mem, nmem) && !pr_overlap(r.p, r.n, o_pre, pix * nh), "stlstm_gates: an input overlaps "
               "an output");
  HR_REQUIRE(!pr_overlap(o_pre, pix * nh, mem, nmem) && !pr_overlap(o_pre, pix * nh, c_t, pix * ldc) &&
             !pr_overlap(o_pre, pix * nh, m_t, pix * ldmt), "stlstm_gates: o_pre overlaps a state or mem");
  a.xc = xc; a.hc = hc; a.mc = mc; a.stats = stats;
  a.wx = wx; a.bx = bx; a.wh = wh; a.bh = bh; a.wm = wm; a.bm = bm;
  a.c_t = c_t; a.m_t = m_t; a.mem = mem; a.o_pre = o_pre;
  a.ldc = ldc; a.c_off = c_off; a.ldmt = ldmt; a.m_off = m_off; a.ldmem = ldmem;
  a.B = B; a.nh = nh; a.q = nh / 4;
  const long long blocks = (a.total + PRG_THREADS - 1) / PRG_THREADS;
  hipLaunchKernelGGL(prg_gates_kernel, dim3((unsigned)blocks), dim3(PRG_THREADS), 0, (hipStream_t)stream, a);
  return hr_check_launch("stlstm_gates");
}

extern "C" int hrnet_stlstm_out(const float* oc, const float* stats, const float* wo, const float* bo, const float* o_pre,
                                const float* last, float* h_new, int B, int H, int W, int nh, hr_stream_t stream) {
  ProArgs a;
  HR_REQUIRE(oc && stats && wo && bo && o_pre && last && h_new, "stlstm_out: null argument");
  int rc = prg_shape("stlstm_out", B, H, W, nh, &a.HW, &a.total);
  if (rc) return rc;
  const void* al[] = {oc, wo, bo, o_pre, last, h_new};
  for (const void* p : al) HR_REQUIRE(pr_aligned16(p), "stlstm_out: every map must be 16-byte aligned");
  const long long nmap = a.HW * B * nh;
  const struct { const void* p; long long n; } in[] = {{oc, nmap}, {stats, 2LL * B}, {wo, a.HW * nh}, {bo, a.HW * nh},
                                                        {o_pre, nmap}, {last, nmap}};
  for (const auto& r : in) HR_REQUIRE(!pr_overlap(r.p, r.n, h_new, nmap), "stlstm_out: an input overlaps h_new");
  a.oc = oc; a.stats = stats; a.wo = wo; a.bo = bo; a.o_pre = o_pre; a.last = last; a.h_new = h_new;
  a.nh = nh; a.q = nh / 4;
  const long long blocks = (a.total + PRG_THREADS - 1) / PRG_THREADS;
  hipLaunchKernelGGL(prg_out_kernel, dim3((unsigned)blocks), dim3(PRG_THREADS), 0, (hipStream_t)stream, a);
  return hr_check_launch("stlstm_out");
}

extern "C" int hrnet_maxpool2d_2x2(const float* x, float* y, int N, int H, int W, int C, int ldx, int x_off, int ldy, int y_off,
                                   hr_stream_t stream) {
  PrpArgs a;
  HR_REQUIRE(x && y, "maxpool2d_2x2: null argument");
  HR_REQUIRE(pr_aligned16(x) && pr_aligned16(y), "maxpool2d_2x2: the maps must be 16-byte aligned");
  HR_REQUIRE(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "maxpool2d_2x2: N = %d, H = %d, W = %d: needs N >= 1 and "
             "even H, W >= 2", N, H, W);
  HR_REQUIRE(C >= 4 && C % 4 == 0 && ldx % 4 == 0 && x_off % 4 == 0 && ldy % 4 == 0 && y_off % 4 == 0, "maxpool2d_2x2: C = %d, "
             "ldx = %d, x_off = %d, ldy = %d, y_off = %d: expected multiples of 4", C, ldx, x_off, ldy, y_off);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + C <= ldx, "maxpool2d_2x2: channels [%d, %d + %d) outside ldx = %d", x_off, x_off,
             C, ldx);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + C <= ldy, "maxpool2d_2x2: channels [%d, %d + %d) outside ldy = %d", y_off, y_off,
             C, ldy);
  HR_REQUIRE((long long)H * W <= 0x7fffffffLL / N, "maxpool2d_2x2: N = %d maps of %d x %d: too many pixels for one launch", N, H,
             W);
  const long long pin = (long long)H * W * N, pout = pin / 4;
  HR_REQUIRE(pout <= (0x7fffffffLL * (PRG_THREADS / 2)) / C && pin <= 0x7fffffffffffLL / ldx && pout <= 0x7fffffffffffLL / ldy,
             "maxpool2d_2x2: N = %d maps of %d x %d x %d: too many elements for one launch", N, H, W, C);
  HR_REQUIRE(!pr_overlap(x, pin * ldx, y, pout * ldy), "maxpool2d_2x2: x and y overlap");
  a.x = x; a.y = y; a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2; a.q = C / 4;
  a.ldx = ldx; a.x_off = x_off; a.ldy = ldy; a.y_off = y_off;
  a.total = pout * a.q;
  const long long blocks = (a.total + PRG_THREADS - 1) / PRG_THREADS;
  hipLaunchKernelGGL(prp_pool_kernel, dim3((unsigned)blocks), dim3(PRG_THREADS), 0, (hipStream_t)stream, a);
  return hr_check_launch("maxpool2d_2x2");
}
