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

// ------------------------------------------------------------------------------------------------ forward: conv3x3 + bias + ReLU, fp16 -> fp16
__global__ __launch_bounds__(CH_NT) void conv3x3_relu_f16_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias,
                                                                 f16* __restrict__ out, Vgg16Geom g) {
  __shared__ __attribute__((aligned(16))) f16 As[2][CH_BM * CH_LD];
  __shared__ __attribute__((aligned(16))) f16 Bs[2][CH_BN * CH_LD];
  const ChTile t(g.Cout);
  ConvRow row[2];
  size_t xb[2];
  const f16* wrow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    row[p] = conv_row(t, p, g.M, g.H, g.W, 1, 1, 1, 1);
    xb[p] = (size_t)row[p].b * g.H * g.W * g.Cin;
    wrow[p] = conv_weight_row(w, t.n0 + t.lr + p * 64, g.Cout, g.K);
  }
  TapCursor<CH_BK> cur;
  cur.init(t.lc, g.Cin, 3);
  auto fetch_a = [&](int p) -> f16x8 {
    const int iy = row[p].iy0 + cur.ky, ix = row[p].ix0 + cur.kx;
    if (cur.ky < 3 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
      return *(const f16x8*)(x + xb[p] + ((size_t)iy * g.W + ix) * g.Cin + cur.ci);
    return (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  };
  auto fetch_b = [&](int p, int k0) { return fetch_weight_row<f16x8>(wrow[p], k0 + t.lc, g.K); };
  auto advance = [&]() { cur.step(g.Cin, 3); };

  f32x4 acc[4][4];
  conv_igemm_f16_mainloop(As, Bs, (g.K + CH_BK - 1) / CH_BK, fetch_a, fetch_b, advance, acc);
  // out = fp16_sat(max(acc + bias, 0)); NaN stays NaN
  CONV_EPILOGUE(acc, 4, t, g.M, g.Cout, conv_bias(bias), [&](int m, int n, float a, float bn) {
    const float v = a + bn;
    out[(size_t)m * g.Cout + n] = to_f16_sat(v > 0.f ? v : (v == v ? 0.f : v));
  });
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
  return conv_launch<CH_BM, CH_BN, CH_NT>("conv3x3_relu_nhwc_f16", conv3x3_relu_f16_kernel, M, Cout, K, stream, (const f16*)x, (const f16*)w, bias, (f16*)out, g);
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
  const ChTile t(g.Cout);
  ConvRow row[2];
  size_t base[2];
  const bf16* wrow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    row[p] = conv_row(t, p, g.M, g.H, g.W, 1, 1, 1, 1);
    base[p] = (size_t)row[p].b * g.H * g.W * g.Cin;
    wrow[p] = conv_weight_row(w, t.n0 + t.lr + p * 64, g.Cout, g.K);
  }
  TapCursor<CH_BK> cur;
  cur.init(t.lc, g.Cin, 3);
  auto fetch_a = [&](int p) -> bf16x8 {
    const int iy = row[p].iy0 + cur.ky, ix = row[p].ix0 + cur.kx;
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
  auto fetch_b = [&](int p, int k0) { return fetch_weight_row<bf16x8>(wrow[p], k0 + t.lc, g.K); };
  auto advance = [&]() { cur.step(g.Cin, 3); };

  f32x4 acc[4][4];
  conv_igemm_f16_mainloop(As, Bs, (g.K + CH_BK - 1) / CH_BK, fetch_a, fetch_b, advance, acc);
  CONV_EPILOGUE(acc, 4, t, g.M, g.Cout, conv_no_col(), [&](int m, int n, float a, int) { dx[(size_t)m * g.Cout + n] = a; });
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
  return conv_launch<CH_BM, CH_BN, CH_NT>("conv3x3_relu_dgrad_bf16", conv3x3_relu_dgrad_bf16_kernel, M, Cx, K, stream, dy, (const f16*)y, (const bf16*)w_rot, dx, g);
}
