// The 3-D convolutions of V2V (reference lib/models/v2v.py): implicit GEMM on the exact-f32 MFMA, a 2x2x2 max-pool
// and the k = 2, s = 2 transposed convolution, forward only, f32 only. Activations are NDHWC with 64-bit offsets.
//
// conv3d / deconv: no LDS. A wave owns kMP groups of 16 consecutive output voxels (in n, d, h, w order, so tiny extents
// and the batch fold into the same walk) and NB blocks of 16 output channels: kMP * NB accumulators of 16 x 16. Per tap
// and per step of 16 (VEC = 4) or 4 (VEC = 1) input channels a lane loads ONE 16-byte (4-byte) fragment per voxel group
// - lane (j = l & 15, g = l >> 4) reads voxel j, channels c0 + g * VEC .. - and one per channel block of the packed
// weights [tap][Cout][Cin]; the same k order on both sides, so every product lands in its sum. A tap is a shift of the
// linear voxel index that is the same for every voxel whose tap lies inside the volume; one outside reads nothing and
// contributes a zero. A tap that lies outside for all of a wave's voxels is skipped (1^3 and 2^3 volumes: most of 3^3).
// The halo is re-read per tap through L1/L2 instead of being staged: DESIGN.md, "V2V inference", says what that costs.
// The accumulator of one output is an fmaf chain in (tap, channel) order whatever the tiling: bit-reproducible.
#include "common.h"

namespace {

constexpr int kMP = 4;            // groups of 16 voxels per wave
constexpr int kWaves = 4;         // waves per workgroup, independent of each other
constexpr int kWaveVox = 16 * kMP;
constexpr int kBlockVox = kWaveVox * kWaves;
constexpr long long kMaxVox = 1LL << 36;

template <int VEC>
struct Frag;
template <>
struct Frag<4> {
  typedef f32x4 type;
  static __device__ __forceinline__ f32x4 zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f32x4 mma(const f32x4& a, const f32x4& b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    return c;
  }
};
template <>
struct Frag<1> {
  typedef float type;
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ f32x4 mma(const float& a, const float& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
};

// DECONV == false: y[n,d,h,w,:] = epilogue(sum over taps and channels), ks^3 taps, zero padding ks / 2.
// DECONV == true: blockIdx.z = (a, b, c) of the 2x2x2 kernel; voxels are INPUT voxels, the tap is that one weight slice
// with no shift, and the result goes to output voxel (2d + a, 2h + b, 2w + c).
template <int NB, int VEC, bool DECONV>
__global__ __launch_bounds__(64 * kWaves) void conv3d_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ res, float* __restrict__ y,
                                                             long long nvox, int D, int H, int W, int Cin, int Cout,
                                                             int ks, int relu) {
  typedef typename Frag<VEC>::type frag_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * (16 * NB);
  const long long base = (long long)blockIdx.x * kBlockVox + (long long)wave * kWaveVox;
  if (base >= nvox) return;                       // the whole wave: MFMA below always runs with every lane on

  long long p[kMP];
  int pd[kMP], ph[kMP], pw[kMP];
#pragma unroll
  for (int m = 0; m < kMP; ++m) {
    p[m] = base + m * 16 + j;
    const long long q = p[m] < nvox ? p[m] : nvox - 1;
    pw[m] = (int)(q % W);
    ph[m] = (int)((q / W) % H);
    pd[m] = (int)((q / ((long long)W * H)) % D);
  }

  f32x4 acc[kMP][NB];
#pragma unroll
  for (int m = 0; m < kMP; ++m)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[m][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int half = ks >> 1;
  const int taps = DECONV ? 1 : ks * ks * ks;
  for (int t = 0; t < taps; ++t) {
    int dd = 0, dh = 0, dw = 0;
    if (!DECONV) {
      dw = t % ks - half;
      dh = (t / ks) % ks - half;
      dd = t / (ks * ks) - half;
    }
    const long long tshift = ((long long)dd * H + dh) * W + dw;
    bool ok[kMP];
    bool any = false;
#pragma unroll
    for (int m = 0; m < kMP; ++m) {
      ok[m] = p[m] < nvox && (unsigned)(pd[m] + dd) < (unsigned)D && (unsigned)(ph[m] + dh) < (unsigned)H &&
              (unsigned)(pw[m] + dw) < (unsigned)W;
      any = any || ok[m];
    }
    if (!__any(any)) continue;                    // wave-uniform: the tap reads only padding
    const int slice = DECONV ? (int)blockIdx.z : t;
    const float* wt = wp + ((long long)slice * Cout + cb + j) * Cin + g * VEC;
    for (int c0 = 0; c0 < Cin; c0 += 4 * VEC) {
      frag_t a[NB], b[kMP];
#pragma unroll
      for (int n = 0; n < NB; ++n) a[n] = *(const frag_t*)(wt + (long long)n * 16 * Cin + c0);
#pragma unroll
      for (int m = 0; m < kMP; ++m)
        b[m] = ok[m] ? *(const frag_t*)(x + (p[m] + tshift) * Cin + c0 + g * VEC) : Frag<VEC>::zero();
#pragma unroll
      for (int m = 0; m < kMP; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = Frag<VEC>::mma(a[n], b[m], acc[m][n]);
    }
  }

  // D layout: column = lane & 15 (voxel), row = 4 * (lane >> 4) + register (channel): a lane stores 4 channels at once
#pragma unroll
  for (int m = 0; m < kMP; ++m) {
    if (p[m] >= nvox) continue;
    long long o = p[m];
    if (DECONV) {
      const int a3 = blockIdx.z;
      const long long n = p[m] / ((long long)W * H * D);
      o = ((n * (2 * D) + 2 * pd[m] + (a3 >> 2)) * (2 * H) + 2 * ph[m] + ((a3 >> 1) & 1)) * (2LL * W) + 2 * pw[m] +
          (a3 & 1);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int c = cb + n * 16 + 4 * g;
      const f32x4 sc = scale ? *(const f32x4*)(scale + c) : f32x4{1.f, 1.f, 1.f, 1.f};
      const f32x4 sh = *(const f32x4*)(shift + c);
      f32x4 v = acc[m][n];
      v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
      if (!DECONV && res) v += *(const f32x4*)(res + o * Cout + c);
      if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      if (DECONV && res) v += *(const f32x4*)(res + o * Cout + c);     // the decoder's upsample(x) + skip: after the ReLU
      *(f32x4*)(y + o * Cout + c) = v;
    }
  }
}

// out[tap][co][ci] (co < Cout_pad, ci < Cin_pad, zero beyond the real counts) from Conv3d's [Cout][Cin][taps] or, with
// transposed != 0, ConvTranspose3d's [Cin][Cout][taps]
__global__ __launch_bounds__(256) void pack_weights3d_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                             int Cout, int Cin, int taps, int Cout_pad, int Cin_pad,
                                                             int transposed, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ci = (int)(i % Cin_pad), co = (int)((i / Cin_pad) % Cout_pad), t = (int)(i / ((long long)Cin_pad * Cout_pad));
  float v = 0.f;
  if (ci < Cin && co < Cout)
    v = transposed ? w[((long long)ci * Cout + co) * taps + t] : w[((long long)co * Cin + ci) * taps + t];
  out[i] = v;
}

// one thread per output voxel and 4 channels; the maximum starts from the first element, not from zero
__global__ __launch_bounds__(256) void maxpool3d_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        long long total, int Do, int Ho, int Wo, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = C >> 2;
  const int c = (int)(i % c4) * 4;
  long long q = i / c4;
  const int w = (int)(q % Wo); q /= Wo;
  const int h = (int)(q % Ho); q /= Ho;
  const int d = (int)(q % Do);
  const long long n = q / Do;
  const int H = 2 * Ho, W = 2 * Wo;
  const long long first = (((n * (2 * Do) + 2 * d) * H + 2 * h) * (long long)W + 2 * w) * C + c;
  f32x4 m = *(const f32x4*)(x + first);
#pragma unroll
  for (int t = 1; t < 8; ++t) {
    const long long at = first + (((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1)) * C;
    const f32x4 v = *(const f32x4*)(x + at);
    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
  }
  *(f32x4*)(y + i * 4) = m;
}

int c3_channels_ok(int Cin, int Cout) {
  return Cin >= 4 && Cin % 4 == 0 && Cout >= 16 && Cout % 16 == 0 && Cin <= 4096 && Cout <= 4096;
}

// a * b * c * d of positive ints, or kMaxVox + 1 once it passes kMaxVox (the plain product overflows 64 bits)
long long c3_product(int a, int b, int c, int d) {
  long long r = a;
  for (const int f : {b, c, d}) {
    r *= f;                                       // r <= 2^36 and f < 2^31: the product stays under 2^63
    if (r > kMaxVox) return kMaxVox + 1;
  }
  return r;
}

int c3_check(const char* what, int dtype, int N, int D, int H, int W, int Cin, int Cout, long long* nvox) {
  HR_REQUIRE(dtype == HR_F32, "%s: dtype = %d: only f32 (HR_F32 = 0) is built", what, dtype);
  HR_REQUIRE(N >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: N = %d, D = %d, H = %d, W = %d", what, N, D, H, W);
  HR_REQUIRE(c3_channels_ok(Cin, Cout), "%s: Cin = %d (a multiple of 4, 4..4096), Cout = %d (a multiple of 16, 16..4096)",
             what, Cin, Cout);
  *nvox = c3_product(N, D, H, W);
  HR_REQUIRE(*nvox <= kMaxVox, "%s: N * D * H * W = more than 2^36 voxels (N = %d, D = %d, H = %d, W = %d)", what, N, D,
             H, W);
  return HR_OK;
}

// output-channel blocks per wave: 4 when they divide Cout, else 2, else 1
int c3_nb(int Cout) { return Cout % 64 == 0 ? 4 : (Cout % 32 == 0 ? 2 : 1); }

template <bool DECONV>
int c3_launch(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y,
              long long nvox, int D, int H, int W, int Cin, int Cout, int ks, int relu, hipStream_t s) {
  const int nb = c3_nb(Cout);
  const dim3 grid((unsigned)((nvox + kBlockVox - 1) / kBlockVox), (unsigned)(Cout / (16 * nb)), DECONV ? 8u : 1u);
  const dim3 block(64 * kWaves);
#define C3_GO(NB, VEC)                                                                                         \
  hipLaunchKernelGGL((conv3d_kernel<NB, VEC, DECONV>), grid, block, 0, s, x, wp, scale, shift, res, y, nvox, D, H, W, \
                     Cin, Cout, ks, relu)
  if (Cin % 16 == 0) {
    if (nb == 4) C3_GO(4, 4); else if (nb == 2) C3_GO(2, 4); else C3_GO(1, 4);
  } else {
    if (nb == 4) C3_GO(4, 1); else if (nb == 2) C3_GO(2, 1); else C3_GO(1, 1);
  }
#undef C3_GO
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_conv3d_supported(int dtype, int Cin, int Cout, int ks) {
  return dtype == HR_F32 && c3_channels_ok(Cin, Cout) && (ks == 1 || ks == 3 || ks == 7) ? 1 : 0;
}

extern "C" int hrnet_conv3d(int dtype, const void* x, const void* w_packed, const float* scale, const float* shift,
                            const void* res, void* y, int N, int D, int H, int W, int Cin, int Cout, int ks, int relu,
                            hr_stream_t stream) {
  long long nvox = 0;
  const int rc = c3_check("conv3d", dtype, N, D, H, W, Cin, Cout, &nvox);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(ks == 1 || ks == 3 || ks == 7, "conv3d: ks = %d (1, 3 or 7)", ks);
  HR_REQUIRE(x && w_packed && shift && y, "conv3d: null argument");
  HR_REQUIRE(x != y && res != y, "conv3d: y aliases an input");
  c3_launch<false>((const float*)x, (const float*)w_packed, scale, shift, (const float*)res, (float*)y, nvox, D, H, W,
                   Cin, Cout, ks, relu != 0, (hipStream_t)stream);
  return hr_check_launch("conv3d");
}

extern "C" int hrnet_deconv3d_k2s2(int dtype, const void* x, const void* w_packed, const float* scale,
                                   const float* shift, const void* add, void* y, int N, int D, int H, int W, int Cin,
                                   int Cout, int relu, hr_stream_t stream) {
  long long nvox = 0;
  const int rc = c3_check("deconv3d_k2s2", dtype, N, D, H, W, Cin, Cout, &nvox);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(nvox * 8 <= kMaxVox, "deconv3d_k2s2: %lld output voxels (at most 2^36)", nvox * 8);
  HR_REQUIRE(x && w_packed && shift && y, "deconv3d_k2s2: null argument");
  HR_REQUIRE(x != y && add != y, "deconv3d_k2s2: y aliases an input");
  c3_launch<true>((const float*)x, (const float*)w_packed, scale, shift, (const float*)add, (float*)y, nvox, D, H, W,
                  Cin, Cout, 1, relu != 0, (hipStream_t)stream);
  return hr_check_launch("deconv3d_k2s2");
}

extern "C" int hrnet_pack_weights3d(int dtype, const float* w, void* out, int Cout, int Cin, int ks, int Cout_pad,
                                    int Cin_pad, int transposed, hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "pack_weights3d: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(w && out, "pack_weights3d: null argument");
  HR_REQUIRE(ks == 1 || ks == 2 || ks == 3 || ks == 7, "pack_weights3d: ks = %d (1, 3, 7; 2 for the deconvolution)", ks);
  HR_REQUIRE(Cout >= 1 && Cin >= 1 && Cout_pad >= Cout && Cin_pad >= Cin && c3_channels_ok(Cin_pad, Cout_pad),
             "pack_weights3d: Cout = %d in %d, Cin = %d in %d (pads: multiples of 16 and of 4)", Cout, Cout_pad, Cin,
             Cin_pad);
  const int taps = ks * ks * ks;
  const long long total = (long long)taps * Cout_pad * Cin_pad;
  hipLaunchKernelGGL(pack_weights3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (float*)out, Cout, Cin, taps, Cout_pad, Cin_pad, transposed != 0, total);
  return hr_check_launch("pack_weights3d");
}

extern "C" int hrnet_maxpool3d(int dtype, const void* x, void* y, int N, int D, int H, int W, int C,
                               hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "maxpool3d: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(x && y && x != y, "maxpool3d: null or aliased argument");
  HR_REQUIRE(N >= 1 && D >= 2 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0 && C <= 4096,
             "maxpool3d: N = %d, D = %d, H = %d, W = %d, C = %d (a multiple of 4, 4..4096)", N, D, H, W, C);
  HR_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "maxpool3d: D = %d, H = %d, W = %d must be even", D, H, W);
  const long long nvox = c3_product(N, D / 2, H / 2, W / 2);
  HR_REQUIRE(nvox <= kMaxVox, "maxpool3d: more than 2^36 output voxels (N = %d, D = %d, H = %d, W = %d)", N, D, H, W);
  const long long total = nvox * (C / 4);
  HR_REQUIRE(total <= 0xffffffffLL * 256, "maxpool3d: %lld outputs (at most 2^42)", total * 4);
  hipLaunchKernelGGL(maxpool3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)x, (float*)y, total, D / 2, H / 2, W / 2, C);
  return hr_check_launch("maxpool3d");
}
