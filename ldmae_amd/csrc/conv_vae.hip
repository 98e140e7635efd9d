// The convolutional KL-VAE tokenizers (tokenizer/autoencoder.py of the reference: the LDM Encoder / Decoder), NHWC f32, forward only.
//   - GroupNorm statistics per (image, group) and a plain normalise(+SiLU) pass;
//   - 3x3 implicit-GEMM convolution on conv_igemm_f32_mainloop whose operand gather does the work of the passes around it: norm-act
//     (silu(gamma (x - mean) rstd + beta), the conv1 / conv2 of ResnetBlock and conv_out), down (stride 2, zero pad right and bottom only) and
//     up (the operand is read at (y >> 1, x >> 1) of the half-size tensor: nearest 2x upsampling that is never written); epilogue bias +
//     residual;
//   - the same epilogue on a 1x1 convolution (proj_out of AttnBlock);
//   - the row softmax between the two f32 GEMMs of the single-head attention of AttnBlock;
//   - the TF32-class form of the two convolutions (operands rounded once to fp16, f32 accumulation on conv_igemm_f16_mainloop) and the
//     normalise pass that writes fp16 for it.
#include "common.h"
#include "conv_igemm_f32.h"
#include "conv_igemm_f16.h"

// One definition of the normalised operand for the fused gather and the stand-alone pass.
template <bool SILU>
__device__ __forceinline__ float gn_act(float x, float mu, float rs, float ga, float be) {
  const float y = fmaf((x - mu) * rs, ga, be);
  return SILU ? y * fast_sigmoid(y) : y;
}

// ------------------------------------------------------------------------------------------------ GroupNorm statistics
// One block of 256 threads per (image, group); a group is HW pixels x cpg adjacent channels.  Two passes over the group (the second one hits
// the L2): mean first, then the biased variance as the mean of (x - mean)^2, so no cancellation of large sums.  Summation order of either
// pass (blocked, never one serial chain over the group): the cpg channels of a pixel are added first; a thread adds the pixel sums of pixels
// tid, tid + 256, ... serially (at most HW / 256 terms); the block is joined by block_sum of common.h (butterfly, then the four waves pairwise).
template <bool VEC>
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ rstd, int HW, int C,
                                                       int G, float eps) {
  __shared__ float sh[4];
  const int cpg = C / G, b = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
  const float* xb = x + (size_t)b * HW * C + (size_t)g * cpg;
  const float inv_n = 1.f / ((float)HW * (float)cpg);
  float s = 0.f;
  for (int p = tid; p < HW; p += 256) {
    const float* px = xb + (size_t)p * C;
    float t = 0.f;
    if (VEC) {
      for (int j = 0; j < cpg; j += 4) { const float4 v = *(const float4*)(px + j); t += (v.x + v.y) + (v.z + v.w); }
    } else {
      for (int j = 0; j < cpg; ++j) t += px[j];
    }
    s += t;
  }
  const float mu = block_sum(s, sh) * inv_n;
  float q = 0.f;
  for (int p = tid; p < HW; p += 256) {
    const float* px = xb + (size_t)p * C;
    float t = 0.f;
    if (VEC) {
      for (int j = 0; j < cpg; j += 4) {
        const float4 v = *(const float4*)(px + j);
        const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
        t += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    } else {
      for (int j = 0; j < cpg; ++j) { const float d = px[j] - mu; t += d * d; }
    }
    q += t;
  }
  const float var = block_sum(q, sh) * inv_n;
  if (tid == 0) {
    mean[blockIdx.x] = mu;
    rstd[blockIdx.x] = 1.f / sqrtf(var + eps);
  }
}

extern "C" int ldmae_groupnorm_stats_nhwc_f32(const float* x, float* mean, float* rstd, int B, int HW, int C, int G, float eps, void* stream) {
  LDMAE_REQUIRE(x && mean && rstd, "groupnorm_stats_nhwc_f32: null pointer");
  LDMAE_REQUIRE(B > 0 && HW > 0 && C > 0 && G > 0 && eps > 0.f, "groupnorm_stats_nhwc_f32: B=%d HW=%d C=%d G=%d eps=%g must be positive", B, HW, C, G, eps);
  LDMAE_REQUIRE(C % G == 0, "groupnorm_stats_nhwc_f32: %d channels are not divisible into %d groups", C, G);
  LDMAE_REQUIRE((long)B * G < (1L << 31) && (long)HW * (C / G) < (1L << 31), "groupnorm_stats_nhwc_f32: problem too large");
  const bool vec = (C / G) % 4 == 0 && ((uintptr_t)x & 15) == 0;
  if (vec) hipLaunchKernelGGL(gn_stats_kernel<true>, dim3(B * G), dim3(256), 0, as_stream(stream), x, mean, rstd, HW, C, G, eps);
  else hipLaunchKernelGGL(gn_stats_kernel<false>, dim3(B * G), dim3(256), 0, as_stream(stream), x, mean, rstd, HW, C, G, eps);
  LDMAE_CHECK_LAUNCH("groupnorm_stats_nhwc_f32");
  return 0;
}

// out = gamma (x - mean) rstd + beta, then SiLU when asked: the GroupNorm in front of q / k / v (no SiLU), and the two-pass form of norm-act.
template <bool SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out, long n,
                                                       int HW, int C, int G) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C), cpg = C / G;
  const long b = i / ((long)HW * C);
  const int s = (int)b * G + c / cpg;
  out[i] = gn_act<SILU>(x[i], mean[s], rstd[s], gamma[c], beta[c]);
}

extern "C" int ldmae_groupnorm_apply_nhwc_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* out,
                                              int B, int HW, int C, int G, int silu, void* stream) {
  LDMAE_REQUIRE(x && mean && rstd && gamma && beta && out, "groupnorm_apply_nhwc_f32: null pointer");
  LDMAE_REQUIRE(B > 0 && HW > 0 && C > 0 && G > 0, "groupnorm_apply_nhwc_f32: B=%d HW=%d C=%d G=%d must be positive", B, HW, C, G);
  LDMAE_REQUIRE(C % G == 0, "groupnorm_apply_nhwc_f32: %d channels are not divisible into %d groups", C, G);
  const long n = (long)B * HW * C;
  LDMAE_REQUIRE((n + 255) / 256 < (1L << 31) && (long)B * G < (1L << 31), "groupnorm_apply_nhwc_f32: problem too large");
  if (silu) hipLaunchKernelGGL(gn_apply_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, mean, rstd, gamma, beta, out, n, HW, C, G);
  else hipLaunchKernelGGL(gn_apply_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, mean, rstd, gamma, beta, out, n, HW, C, G);
  LDMAE_CHECK_LAUNCH("groupnorm_apply_nhwc_f32");
  return 0;
}

// ------------------------------------------------------------------------------------------------ convolution
// M = B*Ho*Wo output pixels, N = Cout, K = ks*ks*Cin (ks = 3, or 1 for the residual 1x1).  The gather works in a VIRTUAL input frame of
// Hv x Wv pixels: the stored tensor [B, H, W, Cin] itself, or (up) its nearest-neighbour 2x enlargement, read at (iy >> 1, ix >> 1).  A tap
// outside the virtual frame contributes exactly 0 in every mode: under norm-act the reference pads the ACTIVATED tensor, so the zero is
// returned without going through gn_act.
struct VaeGeom {
  int B, H, W, Cin;                   // stored input
  int Hv, Wv, up;                     // virtual frame; up = 1: Hv = 2 H, Wv = 2 W
  int Ho, Wo, Cout, ks, stride, pad;
  int M, K, G, cpg;
};

// NORM 0: raw operand; 1: norm-act with cpg % 4 == 0 (the four channels of a float4 share a group); 2: norm-act, any cpg.
template <int NORM, bool SILU>
__global__ __launch_bounds__(CV_NT) void conv_vae_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ res, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out,
                                                         VaeGeom g) {
  __shared__ __attribute__((aligned(16))) float As[2][CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][CV_BN * CV_LD];
  const CvTile t(g.Cout);
  ConvRow row[2];
  int sb[2];
  const float* xb[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    row[p] = conv_row(t, p, g.M, g.Ho, g.Wo, g.stride, g.stride, g.pad, g.pad);
    xb[p] = x + (size_t)row[p].b * g.H * g.W * g.Cin;
    sb[p] = row[p].b * g.G;
  }
  const float* wrow = conv_weight_row(w, t.n0 + t.lr, g.Cout, g.K);
  int ci = t.lc, kx = 0, ky = 0;                   // Cin % 4 == 0, so a float4 never straddles taps
  TAP_WRAP(ci, kx, ky, g.Cin, g.ks)
  // norm-act: gamma / beta of the four channels and their group, the same for both A rows of a step
  float4 ga = make_float4(0.f, 0.f, 0.f, 0.f), be = ga;
  int gi[4] = {0, 0, 0, 0};
  auto coef = [&]() {
    if (NORM != 0 && ky < g.ks) {
      ga = *(const float4*)(gamma + ci);
      be = *(const float4*)(beta + ci);
      if (NORM == 1) {
        gi[0] = ci / g.cpg;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) gi[j] = (ci + j) / g.cpg;
      }
    }
  };
  coef();
  auto fetch_a = [&](int p, int) -> float4 {
    const int iy = row[p].iy0 + ky, ix = row[p].ix0 + kx;
    if (ky < g.ks && (unsigned)iy < (unsigned)g.Hv && (unsigned)ix < (unsigned)g.Wv) {
      float4 v = *(const float4*)(xb[p] + ((size_t)(iy >> g.up) * g.W + (ix >> g.up)) * g.Cin + ci);
      if (NORM == 1) {
        const float mu = mean[sb[p] + gi[0]], rs = rstd[sb[p] + gi[0]];
        v = make_float4(gn_act<SILU>(v.x, mu, rs, ga.x, be.x), gn_act<SILU>(v.y, mu, rs, ga.y, be.y), gn_act<SILU>(v.z, mu, rs, ga.z, be.z),
                        gn_act<SILU>(v.w, mu, rs, ga.w, be.w));
      } else if (NORM == 2) {
        v = make_float4(gn_act<SILU>(v.x, mean[sb[p] + gi[0]], rstd[sb[p] + gi[0]], ga.x, be.x),
                        gn_act<SILU>(v.y, mean[sb[p] + gi[1]], rstd[sb[p] + gi[1]], ga.y, be.y),
                        gn_act<SILU>(v.z, mean[sb[p] + gi[2]], rstd[sb[p] + gi[2]], ga.z, be.z),
                        gn_act<SILU>(v.w, mean[sb[p] + gi[3]], rstd[sb[p] + gi[3]], ga.w, be.w));
      }
      return v;
    }
    return make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto fetch_b = [&](int k0) { return fetch_weight_row<float4>(wrow, k0 + t.lc, g.K); };
  auto advance = [&]() {
    ci += CV_BK;
    TAP_WRAP(ci, kx, ky, g.Cin, g.ks)
    coef();
  };

  f32x4 acc[4][2];
  conv_igemm_f32_mainloop(As, Bs, (g.K + CV_BK - 1) / CV_BK, fetch_a, fetch_b, advance, acc);
  CONV_EPILOGUE(acc, 2, t, g.M, g.Cout, conv_bias(bias), [&](int m, int n, float a, float bn) {
    float v = a + bn;                                      // out = acc + bias + res
    if (res) v += res[(size_t)m * g.Cout + n];
    out[(size_t)m * g.Cout + n] = v;
  });
}

// (norm, silu) -> instantiation; a norm code without a kernel is refused, never mapped to another one
static int launch_conv_vae(const char* name, int norm, int silu, const float* x, const float* w, const float* bias, const float* res, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, float* out, const VaeGeom& g, void* stream) {
#define LDMAE_VAE_LAUNCH(NORM, SILU) \
  return conv_launch<CV_BM, CV_BN, CV_NT>(name, conv_vae_kernel<NORM, SILU>, g.M, g.Cout, g.K, stream, x, w, bias, res, mean, rstd, gamma, beta, out, g)
  if (norm == 0) LDMAE_VAE_LAUNCH(0, false);
  if (norm == 1 && silu) LDMAE_VAE_LAUNCH(1, true);
  if (norm == 1) LDMAE_VAE_LAUNCH(1, false);
  if (norm == 2 && silu) LDMAE_VAE_LAUNCH(2, true);
  if (norm == 2) LDMAE_VAE_LAUNCH(2, false);
#undef LDMAE_VAE_LAUNCH
  LDMAE_FAIL(LDMAE_ERR_INVALID, "%s: no kernel for norm code %d", name, norm);
}

// What the two precisions of an entry point differ in besides its name: the channel multiple of a 16-byte fragment, the tile, and the row
// limit (the fp16 entries keep one tile of headroom below 2^31).
struct VaeLimits { int mult, bm, bn; long m_max; };
constexpr VaeLimits VAE_F32{4, CV_BM, CV_BN, 1L << 31}, VAE_F16{8, CH_BM, CH_BN, (1L << 31) - CH_BM};

// The argument checks of conv3x3_vae_nhwc_* after the mode's, and the mode's geometry.
static int vae_geom_3x3(const char* name, const VaeLimits& lim, int mode, const void* x, const void* w, const void* out, const float* mean,
                        const float* rstd, const float* gamma, const float* beta, int G, int B, int H, int W, int Cin, int Cout, VaeGeom& g) {
  LDMAE_REQUIRE(x && w && out, "%s: null pointer (only bias and res may be NULL)", name);
  LDMAE_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "%s: B=%d H=%d W=%d Cin=%d Cout=%d must be positive", name, B, H, W, Cin, Cout);
  LDMAE_REQUIRE(Cin % lim.mult == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "%s: Cin=%d must be a multiple of %d and x, w 16-B aligned", name,
                Cin, lim.mult);
  g = VaeGeom{};
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.ks = 3;
  g.Hv = H; g.Wv = W; g.up = 0; g.stride = 1; g.pad = 1; g.Ho = H; g.Wo = W; g.G = 1; g.cpg = Cin;
  if (mode == LDMAE_VAE_NORM_ACT) {
    LDMAE_REQUIRE(mean && rstd && gamma && beta && G > 0, "%s: norm-act needs mean, rstd, gamma, beta and a positive group count", name);
    LDMAE_REQUIRE(Cin % G == 0, "%s: %d channels are not divisible into %d groups", name, Cin, G);
    LDMAE_REQUIRE(((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0, "%s: gamma and beta must be 16-B aligned", name);
    g.G = G; g.cpg = Cin / G;
  } else if (mode == LDMAE_VAE_DOWN) {
    LDMAE_REQUIRE(H >= 2 && W >= 2, "%s: down needs at least 2 x 2 pixels", name);
    g.stride = 2; g.pad = 0; g.Ho = (H + 1 - 3) / 2 + 1; g.Wo = (W + 1 - 3) / 2 + 1;      // pad (0, 1, 0, 1): right and bottom only
  } else if (mode == LDMAE_VAE_UP) {
    g.up = 1; g.Hv = 2 * H; g.Wv = 2 * W; g.Ho = 2 * H; g.Wo = 2 * W;
  }
  const long M = (long)B * g.Ho * g.Wo, K = 9L * Cin;
  LDMAE_REQUIRE(M < lim.m_max && M * Cout < (1L << 40) && (long)B * H * W * Cin < (1L << 40) && K < (1L << 24) &&
                    (long)cdiv(M, lim.bm) * cdiv(Cout, lim.bn) < (1L << 31),
                "%s: problem too large", name);
  g.M = (int)M; g.K = (int)K;
  return 0;
}

// The same for conv1x1_res_nhwc_*: M pixels of one row, so no tap ever leaves the frame.
static int vae_geom_1x1(const char* name, const VaeLimits& lim, const void* x, const void* w, const void* out, int M, int Cin, int Cout, VaeGeom& g) {
  LDMAE_REQUIRE(x && w && out, "%s: null pointer (only bias and res may be NULL)", name);
  LDMAE_REQUIRE(M > 0 && Cin > 0 && Cout > 0, "%s: M=%d Cin=%d Cout=%d must be positive", name, M, Cin, Cout);
  LDMAE_REQUIRE(Cin % lim.mult == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "%s: Cin=%d must be a multiple of %d and x, w 16-B aligned", name,
                Cin, lim.mult);
  LDMAE_REQUIRE((long)M < lim.m_max && (long)M * Cout < (1L << 40) && (long)M * Cin < (1L << 40) && Cin < (1 << 24) &&
                    (long)cdiv(M, lim.bm) * cdiv(Cout, lim.bn) < (1L << 31),
                "%s: problem too large", name);
  g = VaeGeom{};
  g.B = 1; g.H = 1; g.W = M; g.Cin = Cin; g.Cout = Cout; g.ks = 1;
  g.Hv = 1; g.Wv = M; g.up = 0; g.stride = 1; g.pad = 0; g.Ho = 1; g.Wo = M; g.G = 1; g.cpg = Cin;
  g.M = M; g.K = Cin;
  return 0;
}

extern "C" int ldmae_conv3x3_vae_nhwc_f32(int mode, const float* x, const float* w, const float* bias, const float* res, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, int G, int silu, float* out, int B, int H, int W,
                                          int Cin, int Cout, void* stream) {
  const char* name = "conv3x3_vae_nhwc_f32";
  LDMAE_REQUIRE(mode == LDMAE_VAE_PLAIN || mode == LDMAE_VAE_NORM_ACT || mode == LDMAE_VAE_DOWN || mode == LDMAE_VAE_UP,
                "%s: mode %d (0 plain, 1 norm-act, 2 down, 3 up)", name, mode);
  VaeGeom g;
  if (const int rc = vae_geom_3x3(name, VAE_F32, mode, x, w, out, mean, rstd, gamma, beta, G, B, H, W, Cin, Cout, g)) return rc;
  const int norm = mode != LDMAE_VAE_NORM_ACT ? 0 : g.cpg % 4 == 0 ? 1 : 2;
  return launch_conv_vae(name, norm, silu, x, w, bias, res, mean, rstd, gamma, beta, out, g, stream);
}

extern "C" int ldmae_conv1x1_res_nhwc_f32(const float* x, const float* w, const float* bias, const float* res, float* out, int M, int Cin, int Cout,
                                          void* stream) {
  VaeGeom g;
  if (const int rc = vae_geom_1x1("conv1x1_res_nhwc_f32", VAE_F32, x, w, out, M, Cin, Cout, g)) return rc;
  return launch_conv_vae("conv1x1_res_nhwc_f32", 0, 0, x, w, bias, res, nullptr, nullptr, nullptr, nullptr, out, g, stream);
}

// ------------------------------------------------------------------------------------------------ TF32-class convolution (fp16 MFMA)
// The same convolutions with both operands of every product rounded once to fp16 (round to nearest even, saturating at +-65504) and the
// products accumulated in f32 on conv_igemm_f16_mainloop; bias and residual are added in f32 and the output is f32.  Under norm-act the
// operand is fp16(gn_act(x)): normalise and SiLU in f32 by the definition above, then one rounding; a tap outside the frame is exactly 0
// and bypasses the activation.  The weight comes packed as fp16 [Cout, ks, ks, Cin]; Cin % 8 == 0, so a 16-B fp16 fragment never
// straddles a tap.  XF16: the input tensor is already fp16 (what groupnorm_apply_nhwc_f16out wrote: the two-pass form), plain gather only.
// NORM 0: raw operand; 1: norm-act, cpg % 8 == 0 (the eight channels of a fragment share a group); 2: cpg % 4 == 0 (each half of a fragment
// has its own group); 3: norm-act, any cpg.
template <int NORM, bool SILU, bool XF16>
__global__ __launch_bounds__(CH_NT) void conv_vae_f16_kernel(const void* __restrict__ xv, const f16* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ res, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ out, VaeGeom g) {
  __shared__ __attribute__((aligned(16))) f16 As[2][CH_BM * CH_LD];
  __shared__ __attribute__((aligned(16))) f16 Bs[2][CH_BN * CH_LD];
  const ChTile t(g.Cout);
  ConvRow row[2];
  int sb[2];
  size_t xb[2];
  const f16* wrow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    row[p] = conv_row(t, p, g.M, g.Ho, g.Wo, g.stride, g.stride, g.pad, g.pad);
    xb[p] = (size_t)row[p].b * g.H * g.W * g.Cin;
    sb[p] = row[p].b * g.G;
    wrow[p] = conv_weight_row(w, t.n0 + t.lr + p * 64, g.Cout, g.K);
  }
  int ci = t.lc, kx = 0, ky = 0;
  TAP_WRAP(ci, kx, ky, g.Cin, g.ks)
  // norm-act: gamma / beta of the eight channels and their groups, the same for both A rows of a step
  float ga[8], be[8];
  int gi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto coef = [&]() {
    if (NORM != 0 && ky < g.ks) {
      const float4 g0 = *(const float4*)(gamma + ci), g1 = *(const float4*)(gamma + ci + 4);
      const float4 b0 = *(const float4*)(beta + ci), b1 = *(const float4*)(beta + ci + 4);
      ga[0] = g0.x; ga[1] = g0.y; ga[2] = g0.z; ga[3] = g0.w; ga[4] = g1.x; ga[5] = g1.y; ga[6] = g1.z; ga[7] = g1.w;
      be[0] = b0.x; be[1] = b0.y; be[2] = b0.z; be[3] = b0.w; be[4] = b1.x; be[5] = b1.y; be[6] = b1.z; be[7] = b1.w;
      if (NORM == 1) {
        gi[0] = ci / g.cpg;
      } else if (NORM == 2) {
        gi[0] = ci / g.cpg;
        gi[4] = (ci + 4) / g.cpg;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) gi[j] = (ci + j) / g.cpg;
      }
    }
  };
  coef();
  auto fetch_a = [&](int p) -> f16x8 {
    const int iy = row[p].iy0 + ky, ix = row[p].ix0 + kx;
    f16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ky < g.ks && (unsigned)iy < (unsigned)g.Hv && (unsigned)ix < (unsigned)g.Wv) {
      const size_t off = xb[p] + ((size_t)(iy >> g.up) * g.W + (ix >> g.up)) * g.Cin + ci;
      if (XF16) return *(const f16x8*)((const f16*)xv + off);
      const float* px = (const float*)xv + off;
      const float4 v0 = *(const float4*)px, v1 = *(const float4*)(px + 4);
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      if (NORM != 0) {
        float mu[8], rs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int jj = NORM == 1 ? 0 : NORM == 2 ? (j & 4) : j;
          if (j == jj) { mu[j] = mean[sb[p] + gi[j]]; rs[j] = rstd[sb[p] + gi[j]]; }
          else { mu[j] = mu[jj]; rs[j] = rs[jj]; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gn_act<SILU>(v[j], mu[j], rs[j], ga[j], be[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = to_f16_sat(v[j]);
    }
    return r;
  };
  auto fetch_b = [&](int p, int k0) { return fetch_weight_row<f16x8>(wrow[p], k0 + t.lc, g.K); };
  auto advance = [&]() {
    ci += CH_BK;
    TAP_WRAP(ci, kx, ky, g.Cin, g.ks)
    coef();
  };

  f32x4 acc[4][4];
  conv_igemm_f16_mainloop(As, Bs, (g.K + CH_BK - 1) / CH_BK, fetch_a, fetch_b, advance, acc);
  CONV_EPILOGUE(acc, 4, t, g.M, g.Cout, conv_bias(bias), [&](int m, int n, float a, float bn) {
    float v = a + bn;                                      // out = acc + bias + res
    if (res) v += res[(size_t)m * g.Cout + n];
    out[(size_t)m * g.Cout + n] = v;
  });
}

static int launch_conv_vae_f16(const char* name, int norm, int silu, bool xf16, const void* x, const void* w, const float* bias, const float* res,
                               const float* mean, const float* rstd, const float* gamma, const float* beta, float* out, const VaeGeom& g,
                               void* stream) {
#define LDMAE_VAE16_LAUNCH(NORM, SILU, XF16)                                                                                                  \
  return conv_launch<CH_BM, CH_BN, CH_NT>(name, conv_vae_f16_kernel<NORM, SILU, XF16>, g.M, g.Cout, g.K, stream, x, (const f16*)w, bias, res, mean, \
                                          rstd, gamma, beta, out, g)
  if (norm == 0 && xf16) LDMAE_VAE16_LAUNCH(0, false, true);
  if (norm == 0) LDMAE_VAE16_LAUNCH(0, false, false);
  if (xf16) LDMAE_FAIL(LDMAE_ERR_INVALID, "%s: no kernel for an fp16 input under norm code %d", name, norm);
  if (norm == 1 && silu) LDMAE_VAE16_LAUNCH(1, true, false);
  if (norm == 1) LDMAE_VAE16_LAUNCH(1, false, false);
  if (norm == 2 && silu) LDMAE_VAE16_LAUNCH(2, true, false);
  if (norm == 2) LDMAE_VAE16_LAUNCH(2, false, false);
  if (norm == 3 && silu) LDMAE_VAE16_LAUNCH(3, true, false);
  if (norm == 3) LDMAE_VAE16_LAUNCH(3, false, false);
#undef LDMAE_VAE16_LAUNCH
  LDMAE_FAIL(LDMAE_ERR_INVALID, "%s: no kernel for norm code %d", name, norm);
}

extern "C" int ldmae_conv3x3_vae_nhwc_f16(int mode, int x_dtype, const void* x, const void* w, const float* bias, const float* res, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, int G, int silu, float* out, int B, int H, int W,
                                          int Cin, int Cout, void* stream) {
  const char* name = "conv3x3_vae_nhwc_f16";
  LDMAE_REQUIRE(mode == LDMAE_VAE_PLAIN || mode == LDMAE_VAE_NORM_ACT || mode == LDMAE_VAE_DOWN || mode == LDMAE_VAE_UP,
                "%s: mode %d (0 plain, 1 norm-act, 2 down, 3 up)", name, mode);
  LDMAE_REQUIRE(x_dtype == LDMAE_F32 || x_dtype == LDMAE_F16, "%s: x_dtype %d (LDMAE_F32 or LDMAE_F16)", name, x_dtype);
  LDMAE_REQUIRE(x_dtype == LDMAE_F32 || mode == LDMAE_VAE_PLAIN, "%s: an fp16 input is taken in plain mode only, got mode %d", name, mode);
  VaeGeom g;
  if (const int rc = vae_geom_3x3(name, VAE_F16, mode, x, w, out, mean, rstd, gamma, beta, G, B, H, W, Cin, Cout, g)) return rc;
  const int norm = mode != LDMAE_VAE_NORM_ACT ? 0 : g.cpg % 8 == 0 ? 1 : g.cpg % 4 == 0 ? 2 : 3;
  return launch_conv_vae_f16(name, norm, silu, x_dtype == LDMAE_F16, x, w, bias, res, mean, rstd, gamma, beta, out, g, stream);
}

extern "C" int ldmae_conv1x1_res_nhwc_f16(const float* x, const void* w, const float* bias, const float* res, float* out, int M, int Cin, int Cout,
                                          void* stream) {
  VaeGeom g;
  if (const int rc = vae_geom_1x1("conv1x1_res_nhwc_f16", VAE_F16, x, w, out, M, Cin, Cout, g)) return rc;
  return launch_conv_vae_f16("conv1x1_res_nhwc_f16", 0, 0, false, x, w, bias, res, nullptr, nullptr, nullptr, nullptr, out, g, stream);
}

// groupnorm_apply writing fp16 (saturating, round to nearest even): the first pass of the two-pass form.  The f32 value is gn_act's, so the
// stored number is the rounding of what ldmae_groupnorm_apply_nhwc_f32 stores.  VEC: eight channels per thread (C % 8 == 0, 16-B aligned).
template <bool SILU, bool VEC>
__global__ __launch_bounds__(256) void gn_apply_f16_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, f16* __restrict__ out, long n,
                                                           int HW, int C, int G) {
  const int cpg = C / G;
  if (VEC) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int sbase = (int)(i / ((long)HW * C)) * G;
    const float4 v0 = *(const float4*)(x + i), v1 = *(const float4*)(x + i + 4);
    const float4 g0 = *(const float4*)(gamma + c), g1 = *(const float4*)(gamma + c + 4);
    const float4 b0 = *(const float4*)(beta + c), b1 = *(const float4*)(beta + c + 4);
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const float ga[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float be[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    f16x8 r;
    if (cpg % 8 == 0) {
      const int s = sbase + c / cpg;
      const float mu = mean[s], rs = rstd[s];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = to_f16_sat(gn_act<SILU>(v[j], mu, rs, ga[j], be[j]));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int s = sbase + (c + j) / cpg;
        r[j] = to_f16_sat(gn_act<SILU>(v[j], mean[s], rstd[s], ga[j], be[j]));
      }
    }
    *(f16x8*)(out + i) = r;
  } else {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int s = (int)(i / ((long)HW * C)) * G + c / cpg;
    out[i] = to_f16_sat(gn_act<SILU>(x[i], mean[s], rstd[s], gamma[c], beta[c]));
  }
}

extern "C" int ldmae_groupnorm_apply_nhwc_f16out(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* out,
                                                 int B, int HW, int C, int G, int silu, void* stream) {
  LDMAE_REQUIRE(x && mean && rstd && gamma && beta && out, "groupnorm_apply_nhwc_f16out: null pointer");
  LDMAE_REQUIRE(B > 0 && HW > 0 && C > 0 && G > 0, "groupnorm_apply_nhwc_f16out: B=%d HW=%d C=%d G=%d must be positive", B, HW, C, G);
  LDMAE_REQUIRE(C % G == 0, "groupnorm_apply_nhwc_f16out: %d channels are not divisible into %d groups", C, G);
  LDMAE_REQUIRE(((uintptr_t)out & 1) == 0, "groupnorm_apply_nhwc_f16out: out must be 2-B aligned");
  const long n = (long)B * HW * C;
  LDMAE_REQUIRE((n + 255) / 256 < (1L << 31) && (long)B * G < (1L << 31), "groupnorm_apply_nhwc_f16out: problem too large");
  const bool vec = C % 8 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0;
  f16* o = (f16*)out;
#define LDMAE_GN16_LAUNCH(SILU, VEC, items) \
  hipLaunchKernelGGL((gn_apply_f16_kernel<SILU, VEC>), dim3(cdiv(items, 256)), dim3(256), 0, as_stream(stream), x, mean, rstd, gamma, beta, o, n, HW, C, G)
  if (vec && silu) LDMAE_GN16_LAUNCH(true, true, n / 8);
  else if (vec) LDMAE_GN16_LAUNCH(false, true, n / 8);
  else if (silu) LDMAE_GN16_LAUNCH(true, false, n);
  else LDMAE_GN16_LAUNCH(false, false, n);
#undef LDMAE_GN16_LAUNCH
  LDMAE_CHECK_LAUNCH("groupnorm_apply_nhwc_f16out");
  return 0;
}

// ------------------------------------------------------------------------------------------------ row softmax
// In place on s [rows, ld]: s[r, :cols] = softmax(scale * s[r, :cols]); columns [cols, ld) are set to 0, so the rows can be the K-padded
// operand of the f32 GEMM that follows.  One block per row: maximum, sum of exp(v - max) (expf, not the fast unit), one true division.
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ s, int ld, int cols, float scale) {
  __shared__ float sh[4];
  float* row = s + (size_t)blockIdx.x * ld;
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int j = tid; j < cols; j += 256) mx = fmaxf(mx, row[j] * scale);
  mx = block_max(mx, sh);
  float sum = 0.f;
  for (int j = tid; j < cols; j += 256) {
    const float e = expf(row[j] * scale - mx);
    row[j] = e;
    sum += e;
  }
  sum = block_sum(sum, sh);
  for (int j = tid; j < ld; j += 256) row[j] = j < cols ? row[j] / sum : 0.f;
}

extern "C" int ldmae_softmax_rows_f32(float* s, int ld, int rows, int cols, float scale, void* stream) {
  LDMAE_REQUIRE(s && rows > 0 && cols > 0 && ld >= cols, "softmax_rows_f32: null pointer, empty problem or ld=%d < cols=%d", ld, cols);
  LDMAE_REQUIRE((long)rows * ld < (1L << 40), "softmax_rows_f32: problem too large");      // rows is the grid's x extent: an int always fits
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, as_stream(stream), s, ld, cols, scale);
  LDMAE_CHECK_LAUNCH("softmax_rows_f32");
  return 0;
}
