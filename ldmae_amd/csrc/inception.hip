// FID evaluation: the kernels of pytorch-fid's Inception-v3 feature extractor (tools/calculate_fid.py:64-425 of the reference), NHWC f32.
//   - implicit-GEMM convolution on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32): M = B*Ho*Wo output pixels, N = Cout, K = kh*kw*Cin; the
//     input patch of every K-step is gathered straight from the NHWC activation (no im2col buffer), epilogue bias + ReLU (BatchNorm folded
//     into weight and bias on the host); input and output are channel slices of wider NHWC tensors, so a Mixed block's torch.cat is free;
//   - 3x3 max / average (count_include_pad=False) pools and the global average, on channel slices as well;
//   - uint8 HWC RGB -> bilinear 299x299 (align_corners=False) -> 2x - 1;
//   - f64 feature statistics: sum(x - s) and sum((x - s)(x - s)^T) accumulated over batches, s a fixed shift.
#include "common.h"
#include "conv_igemm_f32.h"

// ------------------------------------------------------------------------------------------------ convolution
// The tile shape and the MFMA main loop are conv_igemm_f32.h, the skeleton around them conv_igemm_common.h.

struct ConvGeom {
  int B, H, W, Cin, ldx, xoff;        // input [B, H, W, ldx], channels [xoff, xoff + Cin)
  int Ho, Wo, Cout, ldo, ooff;        // output [B, Ho, Wo, ldo], channels [ooff, ooff + Cout)
  int kh, kw, sh, sw, ph, pw;
  int M, K;
};

// VEC: Cin, xoff and ldx are multiples of 4 -- four consecutive k of one tap are one aligned float4 of the input.  Otherwise (the 3-channel
// stem conv) every k is decoded and fetched on its own.
template <bool VEC, bool RELU>
__global__ __launch_bounds__(CV_NT) void conv_igemm_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, ConvGeom g) {
  __shared__ __attribute__((aligned(16))) float As[2][CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][CV_BN * CV_LD];
  const CvTile t(g.Cout);
  int iy0[2], ix0[2];
  const float* xb[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const ConvRow r = conv_row(t, p, g.M, g.Ho, g.Wo, g.sh, g.sw, g.ph, g.pw);
    iy0[p] = r.iy0;
    ix0[p] = r.ix0;
    xb[p] = x + (size_t)r.b * g.H * g.W * g.ldx + g.xoff;
  }
  const float* wrow = conv_weight_row(w, t.n0 + t.lr, g.Cout, g.K);
  int ci = t.lc, kx = 0, ky = 0;                           // VEC: (tap, channel) of this thread's first k
  if (VEC) TAP_WRAP(ci, kx, ky, g.Cin, g.kw)
  auto fetch_a = [&](int p, int k0) -> float4 {
    if constexpr (VEC) {
      const int iy = iy0[p] + ky, ix = ix0[p] + kx;
      if (ky < g.kh && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
        return *(const float4*)(xb[p] + ((size_t)iy * g.W + ix) * g.ldx + ci);
      return make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + t.lc + j;
        const int c = k % g.Cin, tap = k / g.Cin, ty = tap / g.kw, tx = tap % g.kw;
        const int iy = iy0[p] + ty, ix = ix0[p] + tx;
        v[j] = (k < g.K && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) ? xb[p][((size_t)iy * g.W + ix) * g.ldx + c] : 0.f;
      }
      return make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  auto fetch_b = [&](int k0) -> float4 {
    const int k = k0 + t.lc;
    if (VEC) return fetch_weight_row<float4>(wrow, k, g.K);      // K % 4 == 0
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = k + j < g.K ? wrow[k + j] : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
  };
  auto advance = [&]() {
    if (VEC) { ci += CV_BK; TAP_WRAP(ci, kx, ky, g.Cin, g.kw) }
  };

  f32x4 acc[4][2];
  conv_igemm_f32_mainloop(As, Bs, (g.K + CV_BK - 1) / CV_BK, fetch_a, fetch_b, advance, acc);
  CONV_EPILOGUE(acc, 2, t, g.M, g.Cout, conv_bias(bias), [&](int m, int n, float a, float bn) {
    const float v = a + bn;
    out[(size_t)m * g.ldo + g.ooff + n] = RELU ? fmaxf(v, 0.f) : v;
  });
}

extern "C" int ldmae_conv2d_nhwc_f32(const float* x, int ldx, int xoff, const float* w, const float* bias, float* out, int ldo, int ooff, int B, int H,
                                     int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int relu, void* stream) {
  LDMAE_REQUIRE(x && w && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0,
                "conv2d_nhwc_f32: bad arguments");
  LDMAE_REQUIRE(xoff >= 0 && xoff + Cin <= ldx && ooff >= 0 && ooff + Cout <= ldo, "conv2d_nhwc_f32: channel slice [%d, %d) of %d in / [%d, %d) of %d out",
                xoff, xoff + Cin, ldx, ooff, ooff + Cout, ldo);
  const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
  LDMAE_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "conv2d_nhwc_f32: kernel %dx%d larger than the padded %dx%d input", kh, kw, H + 2 * ph, W + 2 * pw);
  const long M = (long)B * Ho * Wo, K = (long)kh * kw * Cin;
  LDMAE_REQUIRE(M < (1L << 31) && (long)B * H * W * ldx < (1L << 40) && K < (1L << 24), "conv2d_nhwc_f32: problem too large");
  ConvGeom g{B, H, W, Cin, ldx, xoff, Ho, Wo, Cout, ldo, ooff, kh, kw, sh, sw, ph, pw, (int)M, (int)K};
  const bool vec = Cin % 4 == 0 && xoff % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0;
#define LDMAE_CONV_LAUNCH(VEC, RELU) \
  return conv_launch<CV_BM, CV_BN, CV_NT>("conv2d_nhwc_f32", conv_igemm_f32_kernel<VEC, RELU>, M, Cout, K, stream, x, w, bias, out, g)
  if (vec && relu) LDMAE_CONV_LAUNCH(true, true);
  if (vec) LDMAE_CONV_LAUNCH(true, false);
  if (relu) LDMAE_CONV_LAUNCH(false, true);
  LDMAE_CONV_LAUNCH(false, false);
#undef LDMAE_CONV_LAUNCH
}

// ------------------------------------------------------------------------------------------------ pools
// one thread per output element (b, oy, ox, c); consecutive threads walk the channels (coalesced).  mode 0: max over the window's in-image
// taps (padding never wins); mode 1: average over the in-image taps (count_include_pad=False).
template <int MODE>
__global__ __launch_bounds__(256) void pool_nhwc_kernel(const float* __restrict__ x, int ldx, int xoff, float* __restrict__ out, int ldo, int ooff,
                                                        int B, int H, int W, int C, int Ho, int Wo, int k, int s, int p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Wo * C) return;
  const int c = (int)(i % C);
  const long pix = i / C;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
  const int y0 = oy * s - p, x0 = ox * s - p;
  const float* xb = x + (size_t)b * H * W * ldx + xoff + c;
  float acc = MODE == 0 ? -INFINITY : 0.f;
  int n = 0;
  for (int dy = 0; dy < k; ++dy) {
    const int iy = y0 + dy;
    if ((unsigned)iy >= (unsigned)H) continue;
    for (int dx = 0; dx < k; ++dx) {
      const int ix = x0 + dx;
      if ((unsigned)ix >= (unsigned)W) continue;
      const float v = xb[((size_t)iy * W + ix) * ldx];
      if (MODE == 0) acc = fmaxf(acc, v);
      else acc += v;
      ++n;
    }
  }
  out[(size_t)pix * ldo + ooff + c] = MODE == 0 ? acc : acc / (float)n;
}

extern "C" int ldmae_pool2d_nhwc_f32(int mode, const float* x, int ldx, int xoff, float* out, int ldo, int ooff, int B, int H, int W, int C, int k,
                                     int stride, int pad, void* stream) {
  LDMAE_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0 && pad >= 0 && 2 * pad < k, "pool2d_nhwc_f32: bad arguments");
  LDMAE_REQUIRE(mode == 0 || mode == 1, "pool2d_nhwc_f32: mode %d (0 = max, 1 = average excluding padding)", mode);
  LDMAE_REQUIRE(xoff >= 0 && xoff + C <= ldx && ooff >= 0 && ooff + C <= ldo, "pool2d_nhwc_f32: bad channel slice");
  LDMAE_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "pool2d_nhwc_f32: window larger than the padded input");
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long n = (long)B * Ho * Wo * C;
  if (mode == 0)
    hipLaunchKernelGGL(pool_nhwc_kernel<0>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, ldx, xoff, out, ldo, ooff, B, H, W, C, Ho, Wo, k, stride, pad);
  else
    hipLaunchKernelGGL(pool_nhwc_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, ldx, xoff, out, ldo, ooff, B, H, W, C, Ho, Wo, k, stride, pad);
  LDMAE_CHECK_LAUNCH("pool2d_nhwc_f32");
  return 0;
}

// global average over HW pixels: out[b, c] = mean_p x[b, p, xoff + c]; one thread per (b, c), channels consecutive
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, int ldx, int xoff, float* __restrict__ out, int B, int HW, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * C) return;
  const int c = (int)(i % C), b = (int)(i / C);
  const float* p = x + (size_t)b * HW * ldx + xoff + c;
  float s = 0.f;
  for (int j = 0; j < HW; ++j) s += p[(size_t)j * ldx];
  out[i] = s / (float)HW;
}

extern "C" int ldmae_global_avgpool_nhwc_f32(const float* x, int ldx, int xoff, float* out, int B, int HW, int C, void* stream) {
  LDMAE_REQUIRE(x && out && B > 0 && HW > 0 && C > 0 && xoff >= 0 && xoff + C <= ldx, "global_avgpool_nhwc_f32: bad arguments");
  hipLaunchKernelGGL(global_avgpool_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, as_stream(stream), x, ldx, xoff, out, B, HW, C);
  LDMAE_CHECK_LAUNCH("global_avgpool_nhwc_f32");
  return 0;
}

// ------------------------------------------------------------------------------------------------ pre-processing
// F.interpolate(img / 255, (Ho, Wo), mode="bilinear", align_corners=False) * 2 - 1 on uint8 HWC RGB; ATen's source-index rule
// (UpSample.h area_pixel_compute_source_index): src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out in f32, the upper tap clamped to
// the last row / column.  One thread per output pixel, three channels.
__global__ __launch_bounds__(256) void fid_preprocess_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int B, int H, int W, int Ho, int Wo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Wo) return;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), b = (int)(i / ((long)Wo * Ho));
  const float shf = (float)H / (float)Ho, swf = (float)W / (float)Wo;
  const float sy = fmaxf(shf * (oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(swf * (ox + 0.5f) - 0.5f, 0.f);
  const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fminf(fmaxf(sy - y0, 0.f), 1.f), ly0 = 1.f - ly1, lx1 = fminf(fmaxf(sx - x0, 0.f), 1.f), lx0 = 1.f - lx1;
  const uint8_t* base = img + (size_t)b * H * W * 3;
  const uint8_t *p00 = base + ((size_t)y0 * W + x0) * 3, *p01 = base + ((size_t)y0 * W + x1) * 3;
  const uint8_t *p10 = base + ((size_t)y1 * W + x0) * 3, *p11 = base + ((size_t)y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v00 = (float)p00[c] / 255.f, v01 = (float)p01[c] / 255.f, v10 = (float)p10[c] / 255.f, v11 = (float)p11[c] / 255.f;
    const float v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    out[i * 3 + c] = v * 2.f - 1.f;
  }
}

extern "C" int ldmae_fid_preprocess(const unsigned char* img, float* out, int B, int H, int W, int Ho, int Wo, void* stream) {
  LDMAE_REQUIRE(img && out && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "fid_preprocess: bad arguments");
  hipLaunchKernelGGL(fid_preprocess_kernel, dim3(cdiv((long)B * Ho * Wo, 256)), dim3(256), 0, as_stream(stream), img, out, B, H, W, Ho, Wo);
  LDMAE_CHECK_LAUNCH("fid_preprocess");
  return 0;
}

// ------------------------------------------------------------------------------------------------ feature statistics (f64)
// sum[d] += sum_r (x[r, d] - s[d]);  cross[i, j] += sum_r (x[r, i] - s[i]) (x[r, j] - s[j]), all in f64.  cross: 64 x 64 tiles, 256 threads
// with 4 x 4 accumulators each, 16 feature rows staged in LDS per step.
constexpr int ST_T = 64, ST_R = 16;

__global__ __launch_bounds__(256) void fid_stats_cross_kernel(const float* __restrict__ x, const float* __restrict__ s, double* __restrict__ cross,
                                                              int n, int D) {
  __shared__ double Yi[ST_R][ST_T], Yj[ST_R][ST_T];
  const int tiles = (D + ST_T - 1) / ST_T;
  const int ti = blockIdx.x / tiles, tj = blockIdx.x % tiles;
  const int i0 = ti * ST_T, j0 = tj * ST_T, tid = threadIdx.x;
  const int ty = tid / 16, tx = tid % 16;
  double acc[4][4] = {};
  for (int r0 = 0; r0 < n; r0 += ST_R) {
    for (int e = tid; e < ST_R * ST_T; e += 256) {
      const int rr = e / ST_T, cc = e % ST_T, r = r0 + rr;
      const int ci = i0 + cc, cj = j0 + cc;
      Yi[rr][cc] = (r < n && ci < D) ? (double)x[(size_t)r * D + ci] - (double)s[ci] : 0.0;
      Yj[rr][cc] = (r < n && cj < D) ? (double)x[(size_t)r * D + cj] - (double)s[cj] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < ST_R; ++rr) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = Yi[rr][ty + 16 * u]; b[u] = Yj[rr][tx + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < D && j < D) cross[(size_t)i * D + j] += acc[u][v];
    }
}

__global__ __launch_bounds__(256) void fid_stats_sum_kernel(const float* __restrict__ x, const float* __restrict__ s, double* __restrict__ sum, int n, int D) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const double sd = (double)s[d];
  double acc = 0.0;
  for (int r = 0; r < n; ++r) acc += (double)x[(size_t)r * D + d] - sd;
  sum[d] += acc;
}

extern "C" int ldmae_fid_stats_accumulate(const float* feats, int n, int D, const float* shift, double* sum, double* cross, void* stream) {
  LDMAE_REQUIRE(feats && shift && sum && cross && n > 0 && D > 0 && D <= 65536, "fid_stats_accumulate: bad arguments");
  hipLaunchKernelGGL(fid_stats_sum_kernel, dim3(cdiv(D, 256)), dim3(256), 0, as_stream(stream), feats, shift, sum, n, D);
  const unsigned tiles = cdiv(D, ST_T);
  hipLaunchKernelGGL(fid_stats_cross_kernel, dim3(tiles * tiles), dim3(256), 0, as_stream(stream), feats, shift, cross, n, D);
  LDMAE_CHECK_LAUNCH("fid_stats_accumulate");
  return 0;
}
