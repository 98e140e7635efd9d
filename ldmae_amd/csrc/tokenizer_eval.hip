// Tokenizer evaluation (the reference's evaluate_tokenizer.py: rFID, PSNR, LPIPS and SSIM of VMAE reconstructions), f32 on gfx950.
//   - LPIPS pre-processing: the ScalingLayer of models/lpips.py on input and target, packed as one NHWC batch of 2B with a zero 4th channel;
//   - the LPIPS head of one VGG tap: per-pixel channel normalisation of both halves, the lin-weighted squared difference, the spatial mean;
//   - torchmetrics' SSIM (11-tap Gaussian, sigma 1.5) fused over LDS tiles: the five blurred maps never reach global memory;
//   - the PNG quantisation clamp(127.5 x + 128, 0, 255) -> uint8 of decoded and reference images with the exact integer SSE per image.
// Every per-image reduction is two-stage: block partials in a fixed order, then one final pass per image in a fixed order.  No atomics.
#include "common.h"

// ------------------------------------------------------------------------------------------------ LPIPS pre-processing
// out[n, y, x, c] = (img[c, y, x] - shift[c]) / scale[c] for c < 3, 0 for c = 3; images 0..B-1 from `input`, B..2B-1 from `target`.
// One thread per pixel, one 16-B store.
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ in0, const float* __restrict__ in1, float* __restrict__ out, int B,
                                                         long HW) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2L * B * HW) return;
  const long n = i / HW, p = i % HW;
  const float* src = (n < B ? in0 + n * 3 * HW : in1 + (n - B) * 3 * HW) + p;
  float4 v;
  v.x = (src[0] - (-0.030f)) / 0.458f;
  v.y = (src[HW] - (-0.088f)) / 0.448f;
  v.z = (src[2 * HW] - (-0.188f)) / 0.450f;
  v.w = 0.f;
  *(float4*)(out + i * 4) = v;
}

// The same f32 arithmetic, then ONE rounding to fp16 (round to nearest even, saturating at +-65504), 8 channels per pixel (3 real, 5 zero): the
// Cin % 8 == 0 operand of the fp16 VGG path (lpips_f16.hip).  One thread per pixel, one 16-B store.
__global__ __launch_bounds__(256) void lpips_prep_f16_kernel(const float* __restrict__ in0, const float* __restrict__ in1, f16* __restrict__ out, int B,
                                                             long HW) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2L * B * HW) return;
  const long n = i / HW, p = i % HW;
  const float* src = (n < B ? in0 + n * 3 * HW : in1 + (n - B) * 3 * HW) + p;
  f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  v[0] = to_f16_sat((src[0] - (-0.030f)) / 0.458f);
  v[1] = to_f16_sat((src[HW] - (-0.088f)) / 0.448f);
  v[2] = to_f16_sat((src[2 * HW] - (-0.188f)) / 0.450f);
  *(f16x8*)(out + i * 8) = v;
}

extern "C" int ldmae_lpips_prep_f16(const float* input, const float* target, void* out, int B, int H, int W, void* stream) {
  LDMAE_REQUIRE(input && target && out && B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 40), "lpips_prep_f16: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)out & 15) == 0, "lpips_prep_f16: out must be 16-byte aligned");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(lpips_prep_f16_kernel, dim3(cdiv(2L * B * HW, 256)), dim3(256), 0, as_stream(stream), input, target, (f16*)out, B, HW);
  LDMAE_CHECK_LAUNCH("lpips_prep_f16");
  return 0;
}

extern "C" int ldmae_lpips_prep(const float* input, const float* target, float* out, int B, int H, int W, void* stream) {
  LDMAE_REQUIRE(input && target && out && B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 40), "lpips_prep: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)out & 15) == 0, "lpips_prep: out must be 16-byte aligned");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(lpips_prep_kernel, dim3(cdiv(2L * B * HW, 256)), dim3(256), 0, as_stream(stream), input, target, out, B, HW);
  LDMAE_CHECK_LAUNCH("lpips_prep");
  return 0;
}

// ------------------------------------------------------------------------------------------------ LPIPS head of one tap
// f [2B, h, w, C] NHWC: image b and image B + b are the two halves of pair b.  A pixel is owned by a group of L = min(64, C / 4) lanes of one
// wave, each lane holding V = C / (4 L) float4 of both halves in registers: the two channel norms are group sums (xor shuffles inside the
// group), then d = sum_c w_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 from the same registers -- equal halves give exactly 0.
// grid (chunks, B): block (k, b) walks pixels k * PPB + j * chunks * PPB of image b and writes its sum of d to part[b * chunks + k].
constexpr int LP_NT = 256, LP_MAX_CHUNKS = 128;

// *dst = the sum of acc over a 256-thread block, for the two f32 sums of this file (the LPIPS head, the SSIM tile): wave_sum, then thread 0
// adds the four wave sums as the CHAIN ((w0 + w1) + w2) + w3.  Not block_sum of common.h, whose join is (w0 + w1) + (w2 + w3): another
// rounding, and these kernels' results are recorded with this one.  One call per kernel: `red` (4 floats of LDS) is not reused.
__device__ __forceinline__ void block_chain_sum(float acc, float* red, float* dst) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += red[i];
    *dst = s;
  }
}

template <int C, typename T>
__global__ __launch_bounds__(LP_NT) void lpips_layer_kernel(const T* __restrict__ f, const float* __restrict__ lw, float* __restrict__ part,
                                                            int B, int HW, int chunks) {
#pragma clang fp contract(off)      // a * r0 - c * r1 with both products rounded: equal halves give exactly 0, not the residual of an fma
  constexpr int L = C / 4 < 64 ? C / 4 : 64, V = C / (4 * L), PPB = LP_NT / L;      // lanes per pixel, float4 per lane, pixels per pass
  __shared__ float red[LP_NT / 64];
  const int tid = threadIdx.x, g = tid / L, gl = tid % L;
  const int b = blockIdx.y;
  const T* f0 = f + (size_t)b * HW * C;
  const T* f1 = f + (size_t)(B + b) * HW * C;
  float4 w[V];
#pragma unroll
  for (int v = 0; v < V; ++v) w[v] = *(const float4*)(lw + (v * L + gl) * 4);
  float acc = 0.f;
  for (long p = (long)blockIdx.x * PPB + g; p < HW; p += (long)chunks * PPB) {
    float4 a[V], c[V];
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
    const float r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float dx = a[v].x * r0 - c[v].x * r1, dy = a[v].y * r0 - c[v].y * r1;
      const float dz = a[v].z * r0 - c[v].z * r1, dw = a[v].w * r0 - c[v].w * r1;
      d += w[v].x * dx * dx + w[v].y * dy * dy + w[v].z * dz * dz + w[v].w * dw * dw;
    }
    acc += lane_group_sum<L>(d) * (gl == 0 ? 1.f : 0.f);       // one lane per group counts the pixel
  }
  block_chain_sum(acc, red, part + (size_t)b * chunks + blockIdx.x);
}

// out[b] += (sum over k of part[b, k], in order, f64) / HW
__global__ __launch_bounds__(64) void lpips_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int B, int HW, int chunks) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += (double)part[(size_t)b * chunks + k];
  out[b] += (float)(s / (double)HW);
}

static int lpips_chunks(long HW) { return (int)std::min<long>(LP_MAX_CHUNKS, std::max<long>(1, (HW + 511) / 512)); }

extern "C" long ldmae_lpips_workspace_bytes(int B, int h, int w) { return (long)B * lpips_chunks((long)h * w) * (long)sizeof(float); }

template <typename T>
static int launch_lpips_layer(const char* name, const T* f, const float* lin_w, float* out, int B, int h, int w, int C, void* workspace, void* stream) {
  LDMAE_REQUIRE(f && lin_w && out && workspace && B > 0 && h > 0 && w > 0 && B <= 65535 && (long)h * w < (1L << 31), "%s: bad arguments", name);
  LDMAE_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "%s: C = %d (64, 128, 256 or 512)", name, C);
  LDMAE_REQUIRE(((uintptr_t)f & 15) == 0 && ((uintptr_t)lin_w & 15) == 0, "%s: features and lin weight must be 16-byte aligned", name);
  const int HW = h * w, chunks = lpips_chunks(HW);
  float* part = (float*)workspace;
  const dim3 grid(chunks, B);
  switch (C) {
    case 64: hipLaunchKernelGGL((lpips_layer_kernel<64, T>), grid, dim3(LP_NT), 0, as_stream(stream), f, lin_w, part, B, HW, chunks); break;
    case 128: hipLaunchKernelGGL((lpips_layer_kernel<128, T>), grid, dim3(LP_NT), 0, as_stream(stream), f, lin_w, part, B, HW, chunks); break;
    case 256: hipLaunchKernelGGL((lpips_layer_kernel<256, T>), grid, dim3(LP_NT), 0, as_stream(stream), f, lin_w, part, B, HW, chunks); break;
    default: hipLaunchKernelGGL((lpips_layer_kernel<512, T>), grid, dim3(LP_NT), 0, as_stream(stream), f, lin_w, part, B, HW, chunks); break;
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), part, out, B, HW, chunks);
  LDMAE_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int ldmae_lpips_layer(const float* f, const float* lin_w, float* out, int B, int h, int w, int C, void* workspace, void* stream) {
  return launch_lpips_layer("lpips_layer", f, lin_w, out, B, h, w, C, workspace, stream);
}

// The taps as the fp16 VGG path stores them; every operation after the load is the f32 arithmetic above (fp16 -> f32 is exact).
extern "C" int ldmae_lpips_layer_f16(const void* f, const float* lin_w, float* out, int B, int h, int w, int C, void* workspace, void* stream) {
  return launch_lpips_layer("lpips_layer_f16", (const f16*)f, lin_w, out, B, h, w, C, workspace, stream);
}

// ------------------------------------------------------------------------------------------------ SSIM (torchmetrics 1.x defaults)
// The cropped output pixel (i, j), 5 <= i < H - 5, 5 <= j < W - 5, reads image rows i - 5 .. i + 5 and columns j - 5 .. j + 5 only, so the
// reflect padding never reaches a kept value and is not materialised.  One block per 32 x 32 output tile of one (image, channel) plane:
//   1. the clamped x / y of the 42 x 42 input window minus a per-tile shift (the clamped values of the tile's first output pixel) -> LDS:
//      variances and covariance are the same about any point, and moments about a nearby value cancel less in f32 (a constant image gives
//      exactly 0 and SSIM exactly 1); the means add the shift back;
//   2. horizontal 11-tap pass of x, y, x^2, y^2, xy for the 42 rows x 32 columns -> LDS (5 maps);
//   3. vertical 11-tap pass per output pixel, the SSIM formula, the block's sum -> part[plane, tile].
// Final pass: one thread per image sums its C * tiles partials in order (f64) and divides by C (H - 10) (W - 10).
constexpr int SS_T = 32, SS_R = 5, SS_IN = SS_T + 2 * SS_R, SS_NT = 256;

struct SsimArgs {
  float lo, hi, c1, c2;
  float g[2 * SS_R + 1];
};

__global__ __launch_bounds__(SS_NT) void ssim_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ part, int H,
                                                          int W, int tiles_x, int tiles, SsimArgs a) {
  __shared__ float xs[SS_IN][SS_IN + 1], ys[SS_IN][SS_IN + 1];
  __shared__ float hs[5][SS_IN][SS_T + 1];
  __shared__ float red[SS_NT / 64];
  const int tid = threadIdx.x, plane = blockIdx.y, tile = blockIdx.x;
  const int oy0 = SS_R + (tile / tiles_x) * SS_T, ox0 = SS_R + (tile % tiles_x) * SS_T;       // first output pixel of the tile
  const float* xp = X + (size_t)plane * H * W;
  const float* yp = Y + (size_t)plane * H * W;
  const float shx = fminf(fmaxf(xp[(size_t)oy0 * W + ox0], a.lo), a.hi), shy = fminf(fmaxf(yp[(size_t)oy0 * W + ox0], a.lo), a.hi);
  for (int e = tid; e < SS_IN * SS_IN; e += SS_NT) {
    const int r = e / SS_IN, c = e % SS_IN, iy = oy0 - SS_R + r, ix = ox0 - SS_R + c;
    float xv = 0.f, yv = 0.f;
    if (iy < H && ix < W) {                                // iy, ix >= 0 always; beyond the image only for pixels that are not output
      xv = fminf(fmaxf(xp[(size_t)iy * W + ix], a.lo), a.hi) - shx;
      yv = fminf(fmaxf(yp[(size_t)iy * W + ix], a.lo), a.hi) - shy;
    }
    xs[r][c] = xv;
    ys[r][c] = yv;
  }
  __syncthreads();
  for (int e = tid; e < SS_IN * SS_T; e += SS_NT) {
    const int r = e / SS_T, c = e % SS_T;
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * SS_R + 1; ++t) {
      const float xv = xs[r][c + t], yv = ys[r][c + t], g = a.g[t];
      sx += g * xv;
      sy += g * yv;
      sxx += g * (xv * xv);
      syy += g * (yv * yv);
      sxy += g * (xv * yv);
    }
    hs[0][r][c] = sx;
    hs[1][r][c] = sy;
    hs[2][r][c] = sxx;
    hs[3][r][c] = syy;
    hs[4][r][c] = sxy;
  }
  __syncthreads();
  float acc = 0.f;
  for (int e = tid; e < SS_T * SS_T; e += SS_NT) {
    const int r = e / SS_T, c = e % SS_T;
    if (oy0 + r >= H - SS_R || ox0 + c >= W - SS_R) continue;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2 * SS_R + 1; ++t) {
      const float g = a.g[t];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += g * hs[q][r + t][c];
    }
    const float vx = fmaxf(m[2] - m[0] * m[0], 0.f), vy = fmaxf(m[3] - m[1] * m[1], 0.f), cxy = m[4] - m[0] * m[1];
    const float mx = m[0] + shx, my = m[1] + shy;
    acc += ((2.f * (mx * my) + a.c1) * (2.f * cxy + a.c2)) / ((mx * mx + my * my + a.c1) * (vx + vy + a.c2));
  }
  block_chain_sum(acc, red, part + (size_t)plane * tiles + tile);
}

// out[b] = sum over the C * tiles partials of image b (in order, f64) / (C (H - 10) (W - 10))
__global__ __launch_bounds__(64) void ssim_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int B, long per_image, double count) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (long k = 0; k < per_image; ++k) s += (double)part[(size_t)b * per_image + k];
  out[b] = (float)(s / count);
}

static long ssim_tiles(int H, int W) { return (long)cdiv(H - 2 * SS_R, SS_T) * cdiv(W - 2 * SS_R, SS_T); }

extern "C" long ldmae_ssim_workspace_bytes(int B, int C, int H, int W) {
  if (H < 2 * SS_R + 1 || W < 2 * SS_R + 1) return 0;
  return (long)B * C * ssim_tiles(H, W) * (long)sizeof(float);
}

extern "C" int ldmae_ssim(const float* preds, const float* target, float* out, int B, int C, int H, int W, float lo, float hi, float data_range,
                          void* workspace, void* stream) {
  LDMAE_REQUIRE(preds && target && out && workspace && B > 0 && C > 0 && (long)B * C <= 65535 && (long)H * W < (1L << 31), "ssim: bad arguments");
  LDMAE_REQUIRE(H >= 2 * SS_R + 1 && W >= 2 * SS_R + 1, "ssim: %d x %d image is smaller than the 11 x 11 Gaussian window", H, W);
  LDMAE_REQUIRE(lo <= hi && data_range > 0.f, "ssim: clamp range [%g, %g], data range %g", (double)lo, (double)hi, (double)data_range);
  SsimArgs a;
  a.lo = lo;
  a.hi = hi;
  a.c1 = (0.01f * data_range) * (0.01f * data_range);
  a.c2 = (0.03f * data_range) * (0.03f * data_range);
  // torchmetrics _gaussian: exp(-(d / sigma)^2 / 2) for d = -5 .. 5 in f32, divided by its sum
  float s = 0.f;
  for (int t = 0; t < 2 * SS_R + 1; ++t) {
    const float d = (float)(t - SS_R) / 1.5f;
    a.g[t] = expf(-(d * d) / 2.f);
    s += a.g[t];
  }
  for (int t = 0; t < 2 * SS_R + 1; ++t) a.g[t] /= s;
  const int tiles_x = (int)cdiv(W - 2 * SS_R, SS_T);
  const long tiles = ssim_tiles(H, W);
  LDMAE_REQUIRE(tiles < (1L << 31), "ssim: image too large");
  float* part = (float*)workspace;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)tiles, B * C), dim3(SS_NT), 0, as_stream(stream), preds, target, part, H, W, tiles_x, (int)tiles, a);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), part, out, B, (long)C * tiles,
                     (double)C * (H - 2 * SS_R) * (W - 2 * SS_R));
  LDMAE_CHECK_LAUNCH("ssim");
  return 0;
}

// ------------------------------------------------------------------------------------------------ PNG quantisation + exact SSE
// q(x) = (uint8) trunc(clamp(127.5 x + 128, 0, 255)) with the multiply and the add rounded separately, as torch evaluates the expression.
// One thread per pixel: reads the three NCHW planes of both images, writes both NHWC uint8 pixels and adds (q(d) - q(r))^2 over the three
// channels to its running sum; grid (blocks, B): the block sum goes to part[b * blocks + k] (64-bit), the final pass adds them in order.
// (__fmul_rn / __fadd_rn are plain operators in the HIP headers and were contracted into one v_fma; the pragma is what keeps them apart.)
__device__ __forceinline__ int png_quantize(float x) {
#pragma clang fp contract(off)
  const float p = 127.5f * x;
  const float v = p + 128.f;
  return (int)fminf(fmaxf(v, 0.f), 255.f);
}

constexpr int QZ_NT = 256, QZ_MAX_BLOCKS = 256;

__global__ __launch_bounds__(QZ_NT) void recon_quantize_kernel(const float* __restrict__ dec, const float* __restrict__ ref, uint8_t* __restrict__ dec8,
                                                               uint8_t* __restrict__ ref8, unsigned long long* __restrict__ part, long HW, int blocks) {
  __shared__ unsigned long long red[QZ_NT / 64];
  const int b = blockIdx.y;
  const float* dp = dec + (size_t)b * 3 * HW;
  const float* rp = ref + (size_t)b * 3 * HW;
  uint8_t* d8 = dec8 + (size_t)b * 3 * HW;
  uint8_t* r8 = ref8 + (size_t)b * 3 * HW;
  unsigned long long acc = 0;
  for (long p = (long)blockIdx.x * QZ_NT + threadIdx.x; p < HW; p += (long)blocks * QZ_NT) {
    unsigned s = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int qd = png_quantize(dp[c * HW + p]), qr = png_quantize(rp[c * HW + p]);
      d8[p * 3 + c] = (uint8_t)qd;
      r8[p * 3 + c] = (uint8_t)qr;
      s += (unsigned)((qd - qr) * (qd - qr));
    }
    acc += s;
  }
  acc = block_sum(acc, red);                                // integers: no order to keep
  if (threadIdx.x == 0) part[(size_t)b * blocks + blockIdx.x] = acc;
}

__global__ __launch_bounds__(QZ_NT) void sse_u8_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b8, unsigned long long* __restrict__ part,
                                                       long n, int blocks) {
  __shared__ unsigned long long red[QZ_NT / 64];
  const int b = blockIdx.y;
  const uint8_t* ap = a + (size_t)b * n;
  const uint8_t* bp = b8 + (size_t)b * n;
  unsigned long long acc = 0;
  for (long i = (long)blockIdx.x * QZ_NT + threadIdx.x; i < n; i += (long)blocks * QZ_NT) {
    const int d = (int)ap[i] - (int)bp[i];
    acc += (unsigned)(d * d);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[(size_t)b * blocks + blockIdx.x] = acc;
}

__global__ __launch_bounds__(64) void sse_finish_kernel(const unsigned long long* __restrict__ part, long long* __restrict__ sse, int B, int blocks) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  unsigned long long s = 0;
  for (int k = 0; k < blocks; ++k) s += part[(size_t)b * blocks + k];
  sse[b] = (long long)s;
}

static int qz_blocks(long n) { return (int)std::min<long>(QZ_MAX_BLOCKS, std::max<long>(1, (n + QZ_NT * 4 - 1) / (QZ_NT * 4))); }

extern "C" long ldmae_sse_workspace_bytes(int B, long pixels) { return (long)B * qz_blocks(pixels) * (long)sizeof(unsigned long long); }

extern "C" int ldmae_recon_quantize_psnr(const float* decoded, const float* ref, unsigned char* dec8, unsigned char* ref8, long long* sse, int B,
                                         int H, int W, void* workspace, void* stream) {
  LDMAE_REQUIRE(decoded && ref && dec8 && ref8 && sse && workspace && B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31),
                "recon_quantize_psnr: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sse & 7) == 0, "recon_quantize_psnr: workspace / sse must be 8-byte aligned");
  const long HW = (long)H * W;
  const int blocks = qz_blocks(HW);
  auto* part = (unsigned long long*)workspace;
  hipLaunchKernelGGL(recon_quantize_kernel, dim3(blocks, B), dim3(QZ_NT), 0, as_stream(stream), decoded, ref, dec8, ref8, part, HW, blocks);
  hipLaunchKernelGGL(sse_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), part, sse, B, blocks);
  LDMAE_CHECK_LAUNCH("recon_quantize_psnr");
  return 0;
}

extern "C" int ldmae_sse_u8(const unsigned char* a, const unsigned char* b, long long* sse, int B, long n, void* workspace, void* stream) {
  LDMAE_REQUIRE(a && b && sse && workspace && B > 0 && B <= 65535 && n > 0 && n < (1L << 40), "sse_u8: bad arguments");
  LDMAE_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sse & 7) == 0, "sse_u8: workspace / sse must be 8-byte aligned");
  const int blocks = qz_blocks(n);
  auto* part = (unsigned long long*)workspace;
  hipLaunchKernelGGL(sse_u8_kernel, dim3(blocks, B), dim3(QZ_NT), 0, as_stream(stream), a, b, part, n, blocks);
  hipLaunchKernelGGL(sse_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), part, sse, B, blocks);
  LDMAE_CHECK_LAUNCH("sse_u8");
  return 0;
}
