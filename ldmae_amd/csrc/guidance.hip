// Guidance rules of the sampler (ldmae_amd/guidance.py): cfg, CFG-rescale and APG on the first k channels of a velocity prediction, in ONE
// launch.  The contract is in include/ldmae_hip.h; DESIGN.md section 26 has the launch structure and the measurements.
//
// The plan.  Block b owns sample b: its n_g = k HW guided elements are contiguous (the first k channels of [C, H, W]).  Thread t of the 1024
// owns the 4-element groups t, t + 1024, ... of them, whatever the access width: the vector path brings a group with one 16-byte load (8
// bytes of bf16), the scalar path with up to four element loads, so both paths sum in the SAME order and give the same bits.  cfg needs no
// sum and is one pass.  rescale and apg make two passes over the sample: pass 1 accumulates the sample's sums in f64 (per thread in group
// order, the xor butterfly 32 .. 1 inside a wave, then every thread adds the 16 wave sums as a chain w0 + w1 + ... + w15), pass 2 reads the
// operands again (196 KB per sample at most at the shipped shape: they come back from L2 / MALL) and applies the rule.  No atomics, no
// workspace; the order depends on n_g alone.  Channels k .. C-1 are copied from pos (widened to f32), or left alone when out IS pos.
#include "common.h"

// Every f32 rounding below is written down: no multiply is fused with an add unless it is spelled fmaf (fm_valid.hip has the reasoning).
#pragma clang fp contract(off)

namespace {

constexpr int GD_THREADS = 1024;
constexpr int GD_WAVES = GD_THREADS / 64;

template <typename T, bool VEC> __device__ __forceinline__ void load_group(const T* p, int nv, float (&v)[4]) {
  if constexpr (VEC) {
    if constexpr (sizeof(T) == 4) {
      const float4 a = *(const float4*)p;
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
      const bf16x4 a = *(const bf16x4*)p;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)a[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? to_f<T>(p[j]) : 0.f;
  }
}

template <bool VEC> __device__ __forceinline__ void store_group(float* p, int nv, const float (&v)[4]) {
  if constexpr (VEC) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) p[j] = v[j];
  }
}

// s[j] <- the block's sum of s[j], the same value in every thread: wave_sum, then the chain w0 + w1 + ... + w15 (1024 threads: this kernel's
// own join, not the 256-thread block_sum of common.h)
template <int N> __device__ __forceinline__ void block_sums_f64(double (&s)[N], double* red) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    s[j] = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) red[j * GD_WAVES + (threadIdx.x >> 6)] = s[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double a = red[j * GD_WAVES];
    for (int w = 1; w < GD_WAVES; ++w) a += red[j * GD_WAVES + w];
    s[j] = a;
  }
}

struct GuideArgs {
  const void* pos;
  const void* neg;
  const float* x;
  const float* t;
  float* mom;
  float* out;
  long n, ng;          // elements per sample, guided elements per sample
  float scale, phi, eta, r, beta;
  int copy_rest;       // 0: out is pos, channels k .. C-1 are already in place
};

__device__ __forceinline__ float cfg_term(float p, float q, float s) {
  const float d = p - q;
  return __builtin_fmaf(s, d, q);
}

template <typename T, int RULE, bool VEC>
__global__ __launch_bounds__(GD_THREADS) void guidance_kernel(GuideArgs a) {
  __shared__ double red[4 * GD_WAVES];
  const long b = blockIdx.x;
  const T* P = (const T*)a.pos + b * a.n;
  const T* Q = (const T*)a.neg + b * a.n;
  float* O = a.out + b * a.n;
  const long ng = a.ng, groups = (ng + 3) >> 2;
  const float s = a.scale;

  if constexpr (RULE == LDMAE_GUIDE_CFG) {
    for (long g = threadIdx.x; g < groups; g += GD_THREADS) {
      const long e = g << 2;
      const int nv = (int)(ng - e < 4 ? ng - e : 4);
      float p[4], q[4], o[4];
      load_group<T, VEC>(P + e, nv, p);
      load_group<T, VEC>(Q + e, nv, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = cfg_term(p[j], q[j], s);
      store_group<VEC>(O + e, nv, o);
    }
  } else if constexpr (RULE == LDMAE_GUIDE_RESCALE) {
    // shifted sums: a sample of equal values has variance exactly 0
    const float kp = to_f<T>(P[0]), kq = to_f<T>(Q[0]);
    const double Kp = (double)kp, Kg = (double)cfg_term(kp, kq, s);
    double sum[4] = {0.0, 0.0, 0.0, 0.0};      // sum (p - Kp), sum (p - Kp)^2, sum (g0 - Kg), sum (g0 - Kg)^2
    for (long g = threadIdx.x; g < groups; g += GD_THREADS) {
      const long e = g << 2;
      const int nv = (int)(ng - e < 4 ? ng - e : 4);
      float p[4], q[4];
      load_group<T, VEC>(P + e, nv, p);
      load_group<T, VEC>(Q + e, nv, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nv) {
          const double dp = (double)p[j] - Kp, dg = (double)cfg_term(p[j], q[j], s) - Kg;
          sum[0] += dp;
          sum[1] = __builtin_fma(dp, dp, sum[1]);
          sum[2] += dg;
          sum[3] = __builtin_fma(dg, dg, sum[3]);
        }
      }
    }
    block_sums_f64<4>(sum, red);
    const double nn = (double)ng;
    double vp = (sum[1] - sum[0] * sum[0] / nn) / (nn - 1.0), vg = (sum[3] - sum[2] * sum[2] / nn) / (nn - 1.0);
    vp = vp > 0.0 ? vp : 0.0;
    const double ratio = vg > 0.0 ? sqrt(vp / vg) : 1.0;
    const float f = (float)(1.0 + (double)a.phi * (ratio - 1.0));
    for (long g = threadIdx.x; g < groups; g += GD_THREADS) {
      const long e = g << 2;
      const int nv = (int)(ng - e < 4 ? ng - e : 4);
      float p[4], q[4], o[4];
      load_group<T, VEC>(P + e, nv, p);
      load_group<T, VEC>(Q + e, nv, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = cfg_term(p[j], q[j], s) * f;
      store_group<VEC>(O + e, nv, o);
    }
  } else {
    const float* X = a.x + b * a.n;
    float* M = a.mom ? a.mom + b * ng : nullptr;
    const float beta = a.beta;
    const bool use_m = M != nullptr && beta != 0.f;
    const float omt = 1.f - a.t[b];
    double sum[3] = {0.0, 0.0, 0.0};           // <d, d>, <d, u>, <u, u>
    for (long g = threadIdx.x; g < groups; g += GD_THREADS) {
      const long e = g << 2;
      const int nv = (int)(ng - e < 4 ? ng - e : 4);
      float p[4], q[4], xv[4], m[4] = {0.f, 0.f, 0.f, 0.f};
      load_group<T, VEC>(P + e, nv, p);
      load_group<T, VEC>(Q + e, nv, q);
      load_group<float, VEC>(X + e, nv, xv);
      if (use_m) load_group<float, VEC>(M + e, nv, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nv) {
          float d = p[j] - q[j];
          if (use_m) d = __builtin_fmaf(beta, m[j], d);
          const double dd = (double)d, uu = (double)__builtin_fmaf(omt, p[j], xv[j]);
          sum[0] = __builtin_fma(dd, dd, sum[0]);
          sum[1] = __builtin_fma(dd, uu, sum[1]);
          sum[2] = __builtin_fma(uu, uu, sum[2]);
        }
      }
    }
    block_sums_f64<3>(sum, red);
    const double den = (double)omt * sqrt(sum[0]);
    double gamma = 1.0;
    if (a.r > 0.f && den > 0.0) {
      gamma = (double)a.r / den;
      gamma = gamma < 1.0 ? gamma : 1.0;
    }
    const double c = sum[2] > 0.0 ? sum[1] / sum[2] : 0.0;
    const float ca = (float)(((double)s - 1.0) * gamma), cb = (float)((1.0 - (double)a.eta) * c);
    for (long g = threadIdx.x; g < groups; g += GD_THREADS) {
      const long e = g << 2;
      const int nv = (int)(ng - e < 4 ? ng - e : 4);
      float p[4], q[4], xv[4], m[4] = {0.f, 0.f, 0.f, 0.f}, o[4], dn[4];
      load_group<T, VEC>(P + e, nv, p);
      load_group<T, VEC>(Q + e, nv, q);
      load_group<float, VEC>(X + e, nv, xv);
      if (use_m) load_group<float, VEC>(M + e, nv, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = p[j] - q[j];
        if (use_m) d = __builtin_fmaf(beta, m[j], d);
        const float u = __builtin_fmaf(omt, p[j], xv[j]);
        const float w = __builtin_fmaf(-cb, u, d);
        o[j] = __builtin_fmaf(ca, w, p[j]);
        dn[j] = d;
      }
      store_group<VEC>(O + e, nv, o);
      if (M) store_group<VEC>(M + e, nv, dn);
    }
  }

  if (a.copy_rest) {                            // channels k .. C-1: pos, widened
    const long rest = a.n - ng;                 // a multiple of 4 on the vector path
    if constexpr (VEC) {
      for (long g = threadIdx.x; g < (rest >> 2); g += GD_THREADS) {
        float p[4];
        load_group<T, true>(P + ng + (g << 2), 4, p);
        store_group<true>(O + ng + (g << 2), 4, p);
      }
    } else {
      for (long i = threadIdx.x; i < rest; i += GD_THREADS) O[ng + i] = to_f<T>(P[ng + i]);
    }
  }
}

}  // namespace

extern "C" int ldmae_guidance_combine(int rule, int in_dtype, const void* pos, const void* neg, const float* x, const float* t, float* mom,
                                      float* out, int B, int C, int HW, int k, float scale, float phi, float eta, float norm_threshold,
                                      float momentum, void* stream) {
  LDMAE_REQUIRE(rule == LDMAE_GUIDE_CFG || rule == LDMAE_GUIDE_RESCALE || rule == LDMAE_GUIDE_APG, "guidance_combine: rule %d (0 cfg, 1 rescale, 2 apg)",
                rule);
  LDMAE_REQUIRE(in_dtype == LDMAE_F32 || in_dtype == LDMAE_BF16, "guidance_combine: dtype %d (f32 or bf16)", in_dtype);
  LDMAE_REQUIRE(pos && neg && out && B > 0 && C > 0 && HW > 0, "guidance_combine: null pointer or empty input (B = %d, C = %d, HW = %d)", B, C, HW);
  LDMAE_REQUIRE(k >= 1 && k <= C, "guidance_combine: k = %d guided channels, expected 1 .. C = %d", k, C);
  const long n = (long)C * HW, ng = (long)k * HW;
  const size_t esize = in_dtype == LDMAE_BF16 ? 2 : 4;
  LDMAE_REQUIRE(is_aligned(pos, esize) && is_aligned(neg, esize) && is_aligned(out, 4), "guidance_combine: pos, neg and out must be aligned to their element size");
  const size_t in_bytes = (size_t)B * n * esize, out_bytes = (size_t)B * n * 4;
  const bool alias = (const void*)out == pos;
  LDMAE_REQUIRE(alias ? in_dtype == LDMAE_F32 : disjoint(out, out_bytes, pos, in_bytes), "guidance_combine: out may be pos itself (f32) but must not overlap it otherwise");
  LDMAE_REQUIRE(disjoint(out, out_bytes, neg, in_bytes), "guidance_combine: out overlaps neg");
  if (rule == LDMAE_GUIDE_RESCALE) {
    LDMAE_REQUIRE(phi >= 0.f && phi <= 1.f, "guidance_combine: phi = %g, expected a value in [0, 1]", (double)phi);
    LDMAE_REQUIRE(ng >= 2, "guidance_combine: rescale needs at least two guided elements per sample, got %ld", ng);
  }
  if (rule == LDMAE_GUIDE_APG) {
    LDMAE_REQUIRE(x && t, "guidance_combine: apg needs the state x and the times t");
    LDMAE_REQUIRE(is_aligned(x, 4) && is_aligned(t, 4) && (!mom || is_aligned(mom, 4)), "guidance_combine: x, t and the momentum buffer must be 4-byte aligned");
    LDMAE_REQUIRE(norm_threshold >= 0.f, "guidance_combine: norm_threshold = %g must not be negative", (double)norm_threshold);
    LDMAE_REQUIRE(mom || momentum == 0.f, "guidance_combine: momentum = %g needs the momentum buffer", (double)momentum);
    LDMAE_REQUIRE(disjoint(out, out_bytes, x, out_bytes), "guidance_combine: out overlaps x");
    if (mom) {
      const size_t mb = (size_t)B * ng * 4;
      LDMAE_REQUIRE(disjoint(mom, mb, out, out_bytes) && disjoint(mom, mb, pos, in_bytes) && disjoint(mom, mb, neg, in_bytes) &&
                    disjoint(mom, mb, x, out_bytes), "guidance_combine: the momentum buffer overlaps another operand");
    }
  } else {
    x = nullptr; t = nullptr; mom = nullptr;
  }
  // 4-element accesses: every sample (and its guided part) starts on a multiple of 4 elements of 16-byte (bf16: 8-byte) aligned storage
  const bool vec = HW % 4 == 0 && is_aligned(pos, 4 * esize) && is_aligned(neg, 4 * esize) && is_aligned(out, 16) && (!x || is_aligned(x, 16)) &&
                   (!mom || is_aligned(mom, 16));
  GuideArgs a{pos, neg, x, t, mom, out, n, ng, scale, phi, eta, norm_threshold, momentum, alias ? 0 : 1};
  hipStream_t st = as_stream(stream);
  auto go = [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    auto launch = [&](auto rc) {
      constexpr int R = decltype(rc)::value;
      if (vec) hipLaunchKernelGGL((guidance_kernel<T, R, true>), dim3((unsigned)B), dim3(GD_THREADS), 0, st, a);
      else hipLaunchKernelGGL((guidance_kernel<T, R, false>), dim3((unsigned)B), dim3(GD_THREADS), 0, st, a);
    };
    if (rule == LDMAE_GUIDE_CFG) launch(IC<LDMAE_GUIDE_CFG>{});
    else if (rule == LDMAE_GUIDE_RESCALE) launch(IC<LDMAE_GUIDE_RESCALE>{});
    else launch(IC<LDMAE_GUIDE_APG>{});
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(in_dtype, go)), "guidance_combine: dtype %d (f32 or bf16)", in_dtype);
  LDMAE_CHECK_LAUNCH("guidance_combine");
  return LDMAE_OK;
}
