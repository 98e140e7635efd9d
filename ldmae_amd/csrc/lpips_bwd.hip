// Backward of the LPIPS network (models/lpips.py: VGG16 taps + lin heads) for the stage-3 decoder tuning of train_ae.sh, f32 NHWC on gfx950.
//   - data gradient of y = relu(conv3x3(x, w) + b) (stride 1, pad 1): dx = conv3x3(dy * [y > 0], w_rot) on the exact-f32 MFMA main loop of the
//     forward conv (conv_igemm_f32.h); the ReLU mask is applied while the operand is gathered -- dy and y have one shape, so the gather fetches
//     both and selects: no masking pass, no masked copy of dy;
//   - 2x2 / 2 max-pool backward: one thread per INPUT element, every element of dx written (no memset, no scatter, no atomics);
//   - head backward of one tap: gradient of mean_hw sum_c lin_c (n0_c - n1_c)^2, n = f / (|f| + 1e-10), to either half or both, overwriting or
//     adding into the buffer the pool backward filled;
//   - ScalingLayer backward: NHWC4 gradient -> NCHW [B, 3, H, W] / scale.
// Nothing here uses atomics: every output element has one writer and a fixed summation order, so the backward is bitwise reproducible.
#include "common.h"
#include "conv_igemm_f32.h"

// ------------------------------------------------------------------------------------------------ conv data gradient, ReLU mask in the gather
// M = B*H*W pixels of dx, N = Cx (the forward conv's input channels), K = 9 * Cy (ky, kx, forward output channel).  w_rot [Cx, 3, 3, Cy]:
// w_rot[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci], built once on the host (models/lpips.py: rotate_weight).
struct DgradGeom {
  int B, H, W, Cy, Cx;
  int M, K;
};

__global__ __launch_bounds__(CV_NT) void conv3x3_relu_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w,
                                                                   float* __restrict__ dx, DgradGeom g) {
  __shared__ __attribute__((aligned(16))) float As[2][CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][CV_BN * CV_LD];
  const CvTile t(g.Cx);
  ConvRow row[2];
  size_t base[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    row[p] = conv_row(t, p, g.M, g.H, g.W, 1, 1, 1, 1);
    base[p] = (size_t)row[p].b * g.H * g.W * g.Cy;
  }
  const float* wrow = conv_weight_row(w, t.n0 + t.lr, g.Cx, g.K);
  int ci = t.lc, kx = 0, ky = 0;                           // Cy % 4 == 0: a float4 never straddles taps
  TAP_WRAP(ci, kx, ky, g.Cy, 3)
  auto fetch_a = [&](int p, int) -> float4 {
    const int iy = row[p].iy0 + ky, ix = row[p].ix0 + kx;
    if (ky < 3 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) {
      const size_t o = base[p] + ((size_t)iy * g.W + ix) * g.Cy + ci;
      const float4 d = *(const float4*)(dy + o), a = *(const float4*)(y + o);
      return make_float4(a.x > 0.f ? d.x : 0.f, a.y > 0.f ? d.y : 0.f, a.z > 0.f ? d.z : 0.f, a.w > 0.f ? d.w : 0.f);
    }
    return make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto fetch_b = [&](int k0) { return fetch_weight_row<float4>(wrow, k0 + t.lc, g.K); };
  auto advance = [&]() { ci += CV_BK; TAP_WRAP(ci, kx, ky, g.Cy, 3) };
  f32x4 acc[4][2];
  conv_igemm_f32_mainloop(As, Bs, (g.K + CV_BK - 1) / CV_BK, fetch_a, fetch_b, advance, acc);
  CONV_EPILOGUE(acc, 2, t, g.M, g.Cx, conv_no_col(), [&](int m, int n, float a, int) { dx[(size_t)m * g.Cx + n] = a; });
}

extern "C" int ldmae_conv3x3_relu_dgrad_nhwc_f32(const float* dy, const float* y, const float* w_rot, float* dx, int B, int H, int W, int Cy, int Cx,
                                                 void* stream) {
  LDMAE_REQUIRE(dy && y && w_rot && dx && B > 0 && H > 0 && W > 0 && Cy > 0 && Cx > 0, "conv3x3_relu_dgrad: bad arguments");
  LDMAE_REQUIRE(Cy % 4 == 0, "conv3x3_relu_dgrad: %d gradient channels (a multiple of 4)", Cy);
  LDMAE_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w_rot & 15) == 0, "conv3x3_relu_dgrad: dy, y and w_rot must be 16-byte aligned");
  const long M = (long)B * H * W, K = 9L * Cy;
  LDMAE_REQUIRE(M < (1L << 31) && M * Cy < (1L << 40) && K < (1L << 24), "conv3x3_relu_dgrad: problem too large");
  DgradGeom g{B, H, W, Cy, Cx, (int)M, (int)K};
  return conv_launch<CV_BM, CV_BN, CV_NT>("conv3x3_relu_dgrad", conv3x3_relu_dgrad_kernel, M, Cx, K, stream, dy, y, w_rot, dx, g);
}

// ------------------------------------------------------------------------------------------------ 2x2 / 2 max-pool backward
// One thread per float4 of dx [B, H, W, C]: it re-reads its window of x, finds the maximum -- the FIRST one in (dy, dx) row-major order on a
// tie, NaN counting as a maximum, as ATen's max_pool2d does -- and takes dy if it is that element, else 0.  Rows / columns past 2 floor(H/2),
// 2 floor(W/2) belong to no window: 0.
__device__ __forceinline__ float pool_pick(float v00, float v01, float v10, float v11, int mine, float d) {
  float best = v00;
  int idx = 0;
  if (v01 > best || v01 != v01) { best = v01; idx = 1; }
  if (v10 > best || v10 != v10) { best = v10; idx = 2; }
  if (v11 > best || v11 != v11) { best = v11; idx = 3; }
  return idx == mine ? d : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ dy, const T* __restrict__ x, float* __restrict__ dx, int B,
                                                             int H, int W, int C4, int Ho, int Wo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * H * W * C4) return;
  const int c = (int)(i % C4);
  const long pix = i / C4;
  const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (py < 2 * Ho && px < 2 * Wo) {
    const int oy = py >> 1, ox = px >> 1, mine = (py & 1) * 2 + (px & 1);
    const T* xw = x + ((((size_t)b * H + 2 * oy) * W + 2 * ox) * C4 + c) * 4;
    const float4 v00 = load4f(xw), v01 = load4f(xw + 4 * C4), v10 = load4f(xw + (size_t)W * C4 * 4), v11 = load4f(xw + ((size_t)W * C4 + C4) * 4);
    const float4 d = ((const float4*)dy)[(((size_t)b * Ho + oy) * Wo + ox) * C4 + c];
    o.x = pool_pick(v00.x, v01.x, v10.x, v11.x, mine, d.x);
    o.y = pool_pick(v00.y, v01.y, v10.y, v11.y, mine, d.y);
    o.z = pool_pick(v00.z, v01.z, v10.z, v11.z, mine, d.z);
    o.w = pool_pick(v00.w, v01.w, v10.w, v11.w, mine, d.w);
  }
  ((float4*)dx)[i] = o;
}

template <typename T>
static int launch_maxpool2x2_bwd(const char* name, const float* dy, const T* x, float* dx, int B, int H, int W, int C, void* stream) {
  LDMAE_REQUIRE(x && dx && B > 0 && H > 0 && W > 0 && C > 0 && (long)B * H * W * C < (1L << 40), "%s: bad arguments", name);
  LDMAE_REQUIRE(C % 4 == 0, "%s: %d channels (a multiple of 4)", name, C);
  const int Ho = H / 2, Wo = W / 2;
  LDMAE_REQUIRE(dy || Ho == 0 || Wo == 0, "%s: dy is null", name);     // an image thinner than one window has no dy: dx is all zeros
  LDMAE_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)dx & 15) == 0, "%s: dy, x and dx must be 16-byte aligned", name);
  const long n = (long)B * H * W * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel<T>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), dy, x, dx, B, H, W, C / 4, Ho, Wo);
  LDMAE_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int ldmae_maxpool2x2_bwd_nhwc_f32(const float* dy, const float* x, float* dx, int B, int H, int W, int C, void* stream) {
  return launch_maxpool2x2_bwd("maxpool2x2_bwd", dy, x, dx, B, H, W, C, stream);
}

// x is the fp16 activation the fp16 VGG path pooled; dy and dx stay f32.  The comparisons are the same (fp16 -> f32 is exact).
extern "C" int ldmae_maxpool2x2_bwd_nhwc_xf16(const float* dy, const void* x, float* dx, int B, int H, int W, int C, void* stream) {
  return launch_maxpool2x2_bwd("maxpool2x2_bwd_xf16", dy, (const f16*)x, dx, B, H, W, C, stream);
}

// ------------------------------------------------------------------------------------------------ LPIPS head backward of one tap
// The lane layout of lpips_layer_kernel (tokenizer_eval.hip): a pixel is owned by a group of L = min(64, C / 4) lanes, each holding V float4 of
// both halves.  With s = |f| + 1e-10, n = f / s, t = (2 g_b / hw) lin (n0 - n1) (= dval/dn0 = -dval/dn1):
//   df0 = t / s0 - f0 (t . f0) / (s0^2 |f0|),      df1 = -(t / s1 - f1 (t . f1) / (s1^2 |f1|)).
// A pixel whose channels are all zero in a half gets gradient exactly 0 in that half (torch: NaN, from sqrt's backward at 0).
// d0 / d1 [B, h, w, C]: gradient to the input / target half; null = not wanted.  ACC: add into them instead of overwriting.
constexpr int LB_NT = 256;

template <int C, bool ACC, typename T>
__global__ __launch_bounds__(LB_NT) void lpips_layer_bwd_kernel(const T* __restrict__ f, const float* __restrict__ lw, const float* __restrict__ gout,
                                                                float* __restrict__ d0, float* __restrict__ d1, int B, int HW, int chunks) {
#pragma clang fp contract(off)      // n0 - n1 from two rounded products, as the forward kernel forms it
  constexpr int L = C / 4 < 64 ? C / 4 : 64, V = C / (4 * L), PPB = LB_NT / L;
  const int tid = threadIdx.x, g = tid / L, gl = tid % L;
  const int b = blockIdx.y;
  const T* f0 = f + (size_t)b * HW * C;
  const T* f1 = f + (size_t)(B + b) * HW * C;
  float* o0 = d0 ? d0 + (size_t)b * HW * C : nullptr;
  float* o1 = d1 ? d1 + (size_t)b * HW * C : nullptr;
  const float coef = 2.f * gout[b] / (float)HW;
  float4 w[V];
#pragma unroll
  for (int v = 0; v < V; ++v) w[v] = *(const float4*)(lw + (v * L + gl) * 4);
  for (long p = (long)blockIdx.x * PPB + g; p < HW; p += (long)chunks * PPB) {
    float4 a[V], c[V], t[V];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      a[v] = load4f(f0 + p * C + (v * L + gl) * 4);
      c[v] = load4f(f1 + p * C + (v * L + gl) * 4);
      s0 += a[v].x * a[v].x + a[v].y * a[v].y + a[v].z * a[v].z + a[v].w * a[v].w;
      s1 += c[v].x * c[v].x + c[v].y * c[v].y + c[v].z * c[v].z + c[v].w * c[v].w;
    }
    s0 = lane_group_sum<L>(s0);
    s1 = lane_group_sum<L>(s1);
    const float nrm0 = sqrtf(s0), nrm1 = sqrtf(s1);
    const float r0 = 1.f / (nrm0 + 1e-10f), r1 = 1.f / (nrm1 + 1e-10f);
    float dot0 = 0.f, dot1 = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      t[v].x = coef * w[v].x * (a[v].x * r0 - c[v].x * r1);
      t[v].y = coef * w[v].y * (a[v].y * r0 - c[v].y * r1);
      t[v].z = coef * w[v].z * (a[v].z * r0 - c[v].z * r1);
      t[v].w = coef * w[v].w * (a[v].w * r0 - c[v].w * r1);
      dot0 += t[v].x * a[v].x + t[v].y * a[v].y + t[v].z * a[v].z + t[v].w * a[v].w;
      dot1 += t[v].x * c[v].x + t[v].y * c[v].y + t[v].z * c[v].z + t[v].w * c[v].w;
    }
    dot0 = lane_group_sum<L>(dot0);
    dot1 = lane_group_sum<L>(dot1);
    if (o0) {
      const float k0 = nrm0 > 0.f ? r0 : 0.f, q0 = nrm0 > 0.f ? dot0 * r0 * r0 / nrm0 : 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float4* dst = (float4*)(o0 + p * C + (v * L + gl) * 4);
        float4 r = make_float4(t[v].x * k0 - a[v].x * q0, t[v].y * k0 - a[v].y * q0, t[v].z * k0 - a[v].z * q0, t[v].w * k0 - a[v].w * q0);
        if (ACC) { const float4 e = *dst; r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w; }
        *dst = r;
      }
    }
    if (o1) {
      const float k1 = nrm1 > 0.f ? r1 : 0.f, q1 = nrm1 > 0.f ? dot1 * r1 * r1 / nrm1 : 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float4* dst = (float4*)(o1 + p * C + (v * L + gl) * 4);
        float4 r = make_float4(c[v].x * q1 - t[v].x * k1, c[v].y * q1 - t[v].y * k1, c[v].z * q1 - t[v].z * k1, c[v].w * q1 - t[v].w * k1);
        if (ACC) { const float4 e = *dst; r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w; }
        *dst = r;
      }
    }
  }
}

template <int C, typename T>
static void launch_lpips_layer_bwd(dim3 grid, hipStream_t st, const T* f, const float* lw, const float* g, float* d0, float* d1, int B, int HW,
                                   int chunks, int accumulate) {
  if (accumulate) hipLaunchKernelGGL((lpips_layer_bwd_kernel<C, true, T>), grid, dim3(LB_NT), 0, st, f, lw, g, d0, d1, B, HW, chunks);
  else hipLaunchKernelGGL((lpips_layer_bwd_kernel<C, false, T>), grid, dim3(LB_NT), 0, st, f, lw, g, d0, d1, B, HW, chunks);
}

template <typename T>
static int lpips_layer_bwd_any(const char* name, const T* f, const float* lin_w, const float* g, float* d_input, float* d_target, int B, int h, int w,
                               int C, int accumulate, void* stream) {
  LDMAE_REQUIRE(f && lin_w && g && (d_input || d_target) && B > 0 && h > 0 && w > 0 && B <= 65535 && (long)h * w < (1L << 31), "%s: bad arguments", name);
  LDMAE_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "%s: C = %d (64, 128, 256 or 512)", name, C);
  LDMAE_REQUIRE(((uintptr_t)f & 15) == 0 && ((uintptr_t)lin_w & 15) == 0 && ((uintptr_t)d_input & 15) == 0 && ((uintptr_t)d_target & 15) == 0,
                "%s: features, lin weight and gradients must be 16-byte aligned", name);
  const int HW = h * w, L = C / 4 < 64 ? C / 4 : 64, ppb = LB_NT / L;
  const int chunks = (int)std::min<long>(4096, cdiv(HW, ppb));      // every pixel has one owner: the split only shapes the grid
  const dim3 grid(chunks, B);
  hipStream_t st = as_stream(stream);
  switch (C) {
    case 64: launch_lpips_layer_bwd<64>(grid, st, f, lin_w, g, d_input, d_target, B, HW, chunks, accumulate); break;
    case 128: launch_lpips_layer_bwd<128>(grid, st, f, lin_w, g, d_input, d_target, B, HW, chunks, accumulate); break;
    case 256: launch_lpips_layer_bwd<256>(grid, st, f, lin_w, g, d_input, d_target, B, HW, chunks, accumulate); break;
    default: launch_lpips_layer_bwd<512>(grid, st, f, lin_w, g, d_input, d_target, B, HW, chunks, accumulate); break;
  }
  LDMAE_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int ldmae_lpips_layer_bwd(const float* f, const float* lin_w, const float* g, float* d_input, float* d_target, int B, int h, int w, int C,
                                     int accumulate, void* stream) {
  return lpips_layer_bwd_any("lpips_layer_bwd", f, lin_w, g, d_input, d_target, B, h, w, C, accumulate, stream);
}

// The taps as the fp16 VGG path stores them; gradients stay f32 and every operation after the load is the arithmetic above.
extern "C" int ldmae_lpips_layer_bwd_f16(const void* f, const float* lin_w, const float* g, float* d_input, float* d_target, int B, int h, int w, int C,
                                         int accumulate, void* stream) {
  return lpips_layer_bwd_any("lpips_layer_bwd_f16", (const f16*)f, lin_w, g, d_input, d_target, B, h, w, C, accumulate, stream);
}

// ------------------------------------------------------------------------------------------------ ScalingLayer backward
// g NHWC [B, H, W, LD] (the data gradient of conv1_1; channels 3 .. LD - 1 are padding channels, never read past the first float4) -> out NCHW
// [B, 3, H, W] = g / scale.  LD = 4: the f32 path; LD = 8: the fp16 path, whose conv1_1 takes 8 input channels.
template <int LD>
__global__ __launch_bounds__(256) void lpips_prep_bwd_kernel(const float* __restrict__ g, float* __restrict__ out, int B, long HW) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * HW) return;
  const long n = i / HW, p = i % HW;
  const float4 v = *(const float4*)(g + i * LD);
  float* dst = out + n * 3 * HW + p;
  dst[0] = v.x / 0.458f;
  dst[HW] = v.y / 0.448f;
  dst[2 * HW] = v.z / 0.450f;
}

extern "C" int ldmae_lpips_prep_bwd(const float* g, float* out, int B, int H, int W, void* stream) {
  LDMAE_REQUIRE(g && out && B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 40), "lpips_prep_bwd: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)g & 15) == 0, "lpips_prep_bwd: g must be 16-byte aligned");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(lpips_prep_bwd_kernel<4>, dim3(cdiv((long)B * HW, 256)), dim3(256), 0, as_stream(stream), g, out, B, HW);
  LDMAE_CHECK_LAUNCH("lpips_prep_bwd");
  return 0;
}

extern "C" int ldmae_lpips_prep_bwd_c8(const float* g, float* out, int B, int H, int W, void* stream) {
  LDMAE_REQUIRE(g && out && B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 40), "lpips_prep_bwd_c8: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)g & 15) == 0, "lpips_prep_bwd_c8: g must be 16-byte aligned");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(lpips_prep_bwd_kernel<8>, dim3(cdiv((long)B * HW, 256)), dim3(256), 0, as_stream(stream), g, out, B, HW);
  LDMAE_CHECK_LAUNCH("lpips_prep_bwd_c8");
  return 0;
}
