// The 16-bit VGG path of LPIPS (models/lpips.py, precision="fp16"): the arithmetic of the reference's autocast + GradScaler run without the scaler.
//   - forward 3x3 / pad 1 / stride 1 convolution with bias and ReLU, fp16 NHWC in, fp16 NHWC out: operands fp16 as stored, products exact in f32
//     and accumulated in f32 on conv_igemm_f16_mainloop (v_mfma_f32_16x16x32_f16), bias added in f32, ReLU, ONE rounding to fp16 (round to
//     nearest even, saturating at +-65504) at the store -- the next layer's fetch reads the rounded number for half the bytes;
//   - 2x2 / 2 max pool on fp16 NHWC (max commutes with rounding: exact);
//   - data gradient of that convolution: dx = conv3x3(bf16(dy * [y > 0]), bf16 w_rot) accumulated in f32 on the same main loop with the element
//     type bf16 (v_mfma_f32_16x16x32_bf16), written f32.  dy is f32 in memory and y is the stored fp16 activation: the gather loads 8 f32 of dy
//     and 8 fp16 of y at one offset, selects, and rounds to bf16.  bf16 because the LPIPS gradient scales as 1 / (h w): at 256 x 256 its values
//     sit near fp16's smallest subnormal, and bf16 has f32's exponent range, so no loss scale is carried.
// Summation order is fixed by the shape (no split K, no atomics): the same bits run to run.  The heads, the pool backward and the ScalingLayer
// kernels that read these fp16 activations are the f32 kernels of tokenizer_eval.hip / lpips_bwd.hip instantiated for an fp16 load.
#include "common.h"
#include "conv_igemm_f16.h"

struct Vgg16Geom {
  int B, H, W, Cin, Cout;      // Cin: channels of the gathered operand (x forward, dy backward); Cout: channels written
  int M, K;
};

// The (tap, channel) cursor of a thread's 8-element fragment; C % 8 == 0, so a fragment never straddles a tap.  A BK step may walk over
// several taps (C < BK), hence the loop.
struct TapCursor {
  int ci, kx, ky;
  __device__ __forceinline__ void init(int lc, int C) { ci = lc; kx = 0; ky = 0; wrap(C); }
  __device__ __forceinline__ void wrap(int C) { while (ci >= C) { ci -= C; if (++kx == 3) { kx = 0; ++ky; } } }
  __device__ __forceinline__ void step(int C) { ci += CH_BK; wrap(C); }
};

// ------------------------------------------------------------------------------------------------ forward: conv3x3 + bias + ReLU, fp16 -> fp16
__global__ __launch_bounds__(CH_NT) void conv3x3_relu_f16_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias,
                                                                 f16* __restrict__ out, Vgg16Geom g) {
  __shared__ __attribute__((aligned(16))) f16 As[2][CH_BM * CH_LD];
  __shared__ __attribute__((aligned(16))) f16 Bs[2][CH_BN * CH_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (g.Cout + CH_BN - 1) / CH_BN;
  const int m0 = (int)(blockIdx.x / tiles_n) * CH_BM, n0 = (int)(blockIdx.x % tiles_n) * CH_BN;
  const int lr = tid >> 2, lc = (tid & 3) * 8;
  int iy0[2], ix0[2];
  size_t xb[2];
  const f16* wrow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int m = min(m0 + lr + p * 64, g.M - 1);          // rows past M fetch a real pixel; their results are never stored
    const int ox = m % g.W, t = m / g.W, oy = t % g.H, b = t / g.H;
    iy0[p] = oy - 1;
    ix0[p] = ox - 1;
    xb[p] = (size_t)b * g.H * g.W * g.Cin;
    wrow[p] = w + (size_t)min(n0 + lr + p * 64, g.Cout - 1) * g.K;      // rows past Cout fetch the last filter; never stored
  }
  TapCursor cur;
  cur.init(lc, g.Cin);
  auto fetch_a = [&](int p) -> f16x8 {
    const int iy = iy0[p] + cur.ky, ix = ix0[p] + cur.kx;
    if (cur.ky < 3 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
      return *(const f16x8*)(x + xb[p] + ((size_t)iy * g.W + ix) * g.Cin + cur.ci);
    return (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  };
  auto fetch_b = [&](int p, int k0) -> f16x8 {
    const int k = k0 + lc;                                 // K % 8 == 0
    if (k < g.K) return *(const f16x8*)(wrow[p] + k);
    return (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  };
  auto advance = [&]() { cur.step(g.Cin); };

  f32x4 acc[4][4];
  conv_igemm_f16_mainloop(As, Bs, (g.K + CH_BK - 1) / CH_BK, fetch_a, fetch_b, advance, acc);
  const int q4 = (lane >> 4) * 4, r16 = lane & 15;
  // epilogue: D row (lane >> 4) * 4 + r, column lane & 15 of each 16 x 16 block; out = fp16_sat(max(acc + bias, 0))
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + r16;
    if (n >= g.Cout) continue;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + i * 16 + q4 + r;
        if (m < g.M) {
          const float v = acc[i][j][r] + bn;
          out[(size_t)m * g.Cout + n] = (f16)sat_f16(v > 0.f ? v : (v == v ? 0.f : v), 65504.f);      // NaN stays NaN
        }
      }
  }
}

extern "C" int ldmae_conv3x3_relu_nhwc_f16(const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                           void* stream) {
  LDMAE_REQUIRE(x && w && out, "conv3x3_relu_nhwc_f16: null pointer (only bias may be NULL)");
  LDMAE_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv3x3_relu_nhwc_f16: B=%d H=%d W=%d Cin=%d Cout=%d must be positive", B, H, W, Cin, Cout);
  LDMAE_REQUIRE(Cin % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)out & 1) == 0,
                "conv3x3_relu_nhwc_f16: Cin=%d must be a multiple of 8, x and w 16-B aligned, out 2-B aligned", Cin);
  const long M = (long)B * H * W, K = 9L * Cin;
  LDMAE_REQUIRE(M < (1L << 31) - CH_BM && M * Cout < (1L << 40) && M * Cin < (1L << 40) && K < (1L << 24) &&
                    (long)cdiv(M, CH_BM) * cdiv(Cout, CH_BN) < (1L << 31),
                "conv3x3_relu_nhwc_f16: problem too large");
  Vgg16Geom g{B, H, W, Cin, Cout, (int)M, (int)K};
  const unsigned grid = cdiv(M, CH_BM) * cdiv(Cout, CH_BN);
  const long pidx = ldmae_prof_is_on() ? ldmae_prof_begin(as_stream(stream), 2.0 * M * Cout * K) : -1;
  hipLaunchKernelGGL(conv3x3_relu_f16_kernel, dim3(grid), dim3(CH_NT), 0, as_stream(stream), (const f16*)x, (const f16*)w, bias, (f16*)out, g);
  if (pidx >= 0) ldmae_prof_end(pidx, as_stream(stream));
  LDMAE_CHECK_LAUNCH("conv3x3_relu_nhwc_f16");
  return 0;
}

// ------------------------------------------------------------------------------------------------ 2x2 / 2 max pool, fp16
// One thread per 8 channels of an output pixel (16-B loads and store).  The first maximum in row-major order wins and NaN counts as a maximum,
// as ATen's max_pool2d; the odd last row / column belongs to no window.
__device__ __forceinline__ f16 max_keep_first(f16 best, f16 v) { return (v > best || v != v) ? v : best; }

__global__ __launch_bounds__(256) void maxpool2x2_f16_kernel(const f16* __restrict__ x, f16* __restrict__ out, int B, int H, int W, int C8, int Ho, int Wo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Wo * C8) return;
  const int c = (int)(i % C8);
  const long pix = i / C8;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
  const f16x8* xw = (const f16x8*)x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C8 + c;
  const f16x8 v00 = xw[0], v01 = xw[C8], v10 = xw[(size_t)W * C8], v11 = xw[(size_t)W * C8 + C8];
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = max_keep_first(max_keep_first(max_keep_first(v00[j], v01[j]), v10[j]), v11[j]);
  ((f16x8*)out)[i] = o;
}

extern "C" int ldmae_maxpool2x2_nhwc_f16(const void* x, void* out, int B, int H, int W, int C, void* stream) {
  LDMAE_REQUIRE(x && out && B > 0 && H >= 2 && W >= 2 && C > 0 && (long)B * H * W * C < (1L << 40), "maxpool2x2_nhwc_f16: bad arguments (H, W >= 2)");
  LDMAE_REQUIRE(C % 8 == 0, "maxpool2x2_nhwc_f16: %d channels (a multiple of 8)", C);
  LDMAE_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "maxpool2x2_nhwc_f16: x and out must be 16-byte aligned");
  const int Ho = H / 2, Wo = W / 2;
  const long n = (long)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(maxpool2x2_f16_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), (const f16*)x, (f16*)out, B, H, W, C / 8, Ho, Wo);
  LDMAE_CHECK_LAUNCH("maxpool2x2_nhwc_f16");
  return 0;
}

// ------------------------------------------------------------------------------------------------ data gradient, bf16 operands
// M = B*H*W pixels of dx, N = Cx, K = 9 * Cy (ky, kx, forward output channel); w_rot bf16 [Cx, 3, 3, Cy] (rotate_weight, rounded once per object).
__global__ __launch_bounds__(CH_NT) void conv3x3_relu_dgrad_bf16_kernel(const float* __restrict__ dy, const f16* __restrict__ y, const bf16* __restrict__ w,
                                                                        float* __restrict__ dx, Vgg16Geom g) {
  __shared__ __attribute__((aligned(16))) bf16 As[2][CH_BM * CH_LD];
  __shared__ __attribute__((aligned(16))) bf16 Bs[2][CH_BN * CH_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (g.Cout + CH_BN - 1) / CH_BN;
  const int m0 = (int)(blockIdx.x / tiles_n) * CH_BM, n0 = (int)(blockIdx.x % tiles_n) * CH_BN;
  const int lr = tid >> 2, lc = (tid & 3) * 8;
  int iy0[2], ix0[2];
  size_t base[2];
  const bf16* wrow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int m = min(m0 + lr + p * 64, g.M - 1);          // rows past M fetch a real pixel; their results are never stored
    const int ox = m % g.W, t = m / g.W, oy = t % g.H, b = t / g.H;
    iy0[p] = oy - 1;
    ix0[p] = ox - 1;
    base[p] = (size_t)b * g.H * g.W * g.Cin;
    wrow[p] = w + (size_t)min(n0 + lr + p * 64, g.Cout - 1) * g.K;
  }
  TapCursor cur;
  cur.init(lc, g.Cin);
  auto fetch_a = [&](int p) -> bf16x8 {
    const int iy = iy0[p] + cur.ky, ix = ix0[p] + cur.kx;
    bf16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cur.ky < 3 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) {
      const size_t o = base[p] + ((size_t)iy * g.W + ix) * g.Cin + cur.ci;
      const float4 d0 = *(const float4*)(dy + o), d1 = *(const float4*)(dy + o + 4);
      const f16x8 a = *(const f16x8*)(y + o);
      const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (bf16)(a[j] > (f16)0 ? d[j] : 0.f);
    }
    return r;
  };
  auto fetch_b = [&](int p, int k0) -> bf16x8 {
    const int k = k0 + lc;                                 // K % 8 == 0
    if (k < g.K) return *(const bf16x8*)(wrow[p] + k);
    return (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  };
  auto advance = [&]() { cur.step(g.Cin); };

  f32x4 acc[4][4];
  conv_igemm_f16_mainloop(As, Bs, (g.K + CH_BK - 1) / CH_BK, fetch_a, fetch_b, advance, acc);
  const int q4 = (lane >> 4) * 4, r16 = lane & 15;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + r16;
    if (n >= g.Cout) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + i * 16 + q4 + r;
        if (m < g.M) dx[(size_t)m * g.Cout + n] = acc[i][j][r];
      }
  }
}

extern "C" int ldmae_conv3x3_relu_dgrad_nhwc_bf16(const float* dy, const void* y, const void* w_rot, float* dx, int B, int H, int W, int Cy, int Cx,
                                                  void* stream) {
  LDMAE_REQUIRE(dy && y && w_rot && dx && B > 0 && H > 0 && W > 0 && Cy > 0 && Cx > 0, "conv3x3_relu_dgrad_bf16: bad arguments");
  LDMAE_REQUIRE(Cy % 8 == 0, "conv3x3_relu_dgrad_bf16: %d gradient channels (a multiple of 8)", Cy);
  LDMAE_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w_rot & 15) == 0 && ((uintptr_t)dx & 3) == 0,
                "conv3x3_relu_dgrad_bf16: dy, y and w_rot must be 16-byte aligned");
  const long M = (long)B * H * W, K = 9L * Cy;
  LDMAE_REQUIRE(M < (1L << 31) - CH_BM && M * Cy < (1L << 40) && M * Cx < (1L << 40) && K < (1L << 24) &&
                    (long)cdiv(M, CH_BM) * cdiv(Cx, CH_BN) < (1L << 31),
                "conv3x3_relu_dgrad_bf16: problem too large");
  Vgg16Geom g{B, H, W, Cy, Cx, (int)M, (int)K};
  const unsigned grid = cdiv(M, CH_BM) * cdiv(Cx, CH_BN);
  const long pidx = ldmae_prof_is_on() ? ldmae_prof_begin(as_stream(stream), 2.0 * M * Cx * K) : -1;
  hipLaunchKernelGGL(conv3x3_relu_dgrad_bf16_kernel, dim3(grid), dim3(CH_NT), 0, as_stream(stream), dy, (const f16*)y, (const bf16*)w_rot, dx, g);
  if (pidx >= 0) ldmae_prof_end(pidx, as_stream(stream));
  LDMAE_CHECK_LAUNCH("conv3x3_relu_dgrad_bf16");
  return 0;
}
