// Adaptive Dormand-Prince 5(4) ODE sampler (transport/integrators.py, sampler_type "dopri5"): the solver's own arithmetic between two model
// evaluations.  All f32, plain vector code, every kernel bound by HBM traffic (one pass over its operands, 16-byte accesses).
//
// Layout.  The seven stage derivatives live in one slab k[7][ld] (ld % 4 == 0, ld >= n: every row 16-byte aligned for any n).  A kernel
// walks its n floats with flat_walk of flat_common.h (float4 items plus a scalar tail, a grid that is a function of n alone) and gives it
// the work on one item; dopri5_interp_kernel alone spells the same walk out (the reason stands in it).
//
// Reductions (the error ratio and the norms of the initial-step rule) are two-stage and fixed-order, no atomics: a thread adds its (up to 16)
// squares in element order, block_sum joins the block (DESIGN.md section 27 has the order) and the block stores partial[block]; one block of
// row_fold_kernel folds the partials and writes sqrt(sum / n).  The order depends on n only: two runs give the same bits.
//
// Step size, time and the accept decision stay on the device (ldmae_dopri5_advance): the kernels that read h and the decision taken from the
// error ratio see the same bits, and the host reads one small status record per attempted step.
//
// Likelihood evaluation (transport.Sampler.sample_ode_likelihood) adds the Hutchinson probe and its reductions at the end of this file: the
// Rademacher draw from Philox4x32-10 (Salmon et al., SC'11: a counter-based generator, so the draw is a function of (seed, counter, element)
// alone), the per-sample dot product of two [B, m] tensors, and the last line of the log-likelihood.  Same rules: f32, no atomics, fixed order.
//
// The SDE sampler (transport.Sampler.sample_sde) adds the standard-normal draw from the same generator (Box-Muller on its words) and the one
// launch between two model evaluations of an Euler-Maruyama / Heun step: a linear combination of up to four tensors plus a multiple of the
// draw, the draw generated in the same pass.  Its coefficients come from the host by value: nothing is read back.
#include "flat_common.h"
#include "philox_normal.h"

namespace {

struct RkCoef { float c[7]; };

// c_sol (= row 7 of the tableau: FSAL), c_error = c_sol - the embedded 4th-order weights; b[1] = e[1] = 0 and b[6] = 0
constexpr float DP_B0 = (float)(35.0 / 384.0), DP_B2 = (float)(500.0 / 1113.0), DP_B3 = (float)(125.0 / 192.0), DP_B4 = (float)(-2187.0 / 6784.0),
                DP_B5 = (float)(11.0 / 84.0);
constexpr float DP_E0 = (float)(35.0 / 384.0 - 1951.0 / 21600.0), DP_E2 = (float)(500.0 / 1113.0 - 22642.0 / 50085.0),
                DP_E3 = (float)(125.0 / 192.0 - 451.0 / 720.0), DP_E4 = (float)(-2187.0 / 6784.0 + 12231.0 / 42400.0),
                DP_E5 = (float)(11.0 / 84.0 - 649.0 / 6300.0), DP_E6 = (float)(-1.0 / 60.0);

// ---------------------------------------------------------------- out = y + h * sum_{j < M} coef_j k_j
template <int M> __device__ __forceinline__ float stage1(float y, const float (&k)[7], const RkCoef& cf, float h) {
  float acc = cf.c[0] * k[0];
#pragma unroll
  for (int j = 1; j < M; ++j) acc = __builtin_fmaf(cf.c[j], k[j], acc);
  return __builtin_fmaf(h, acc, y);
}

template <int M>
__global__ __launch_bounds__(FLAT_THREADS) void rk_stage_kernel(const float* __restrict__ y, const float* __restrict__ k, long ld, RkCoef cf,
                                                                const float* __restrict__ h_dev, float* out, long n,
                                                                const float* __restrict__ t_dev, float ct, float* __restrict__ t_out, int nt) {
  const float h = *h_dev;
  if (t_out) flat_fill_side(t_out, nt, __builtin_fmaf(ct, h, *t_dev));      // the time the NEXT model evaluation is fed: t + ct h
  flat_walk(n, true, [&](long v, int cnt, bool whole) {
    float yy[4], kk[M][4], o[4];
    flat_load(y, v, cnt, whole, yy);
#pragma unroll
    for (int j = 0; j < M; ++j) flat_load(k + (long)j * ld, v, cnt, whole, kk[j]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float kj[7];
#pragma unroll
      for (int j = 0; j < M; ++j) kj[j] = kk[j][e];
      o[e] = stage1<M>(yy[e], kj, cf, h);
    }
    flat_store(out, v, cnt, whole, o);
  });
}

// the fold of the per-block partial sums of squares (row_fold_kernel, one block): the root of their mean over the n elements
struct RmsFinish {
  float n;
  __device__ float operator()(float s) const { return sqrtf(s / n); }
};
void launch_rms_fold(const float* partial, unsigned nparts, long n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(row_fold_kernel<RmsFinish>, dim3(1), dim3(FLAT_THREADS), 0, st, partial, (long)nparts, RmsFinish{(float)n}, out);
}

// ---------------------------------------------------------------- y1 = y + h sum b_j k_j; partial[block] = sum (h sum e_j k_j / tol)^2
__device__ __forceinline__ float finish1(float y, float k0, float k2, float k3, float k4, float k5, float k6, float h, float atol, float rtol, float& y1) {
  float acc = DP_B0 * k0;
  acc = __builtin_fmaf(DP_B2, k2, acc);
  acc = __builtin_fmaf(DP_B3, k3, acc);
  acc = __builtin_fmaf(DP_B4, k4, acc);
  acc = __builtin_fmaf(DP_B5, k5, acc);
  y1 = __builtin_fmaf(h, acc, y);
  float e = DP_E0 * k0;
  e = __builtin_fmaf(DP_E2, k2, e);
  e = __builtin_fmaf(DP_E3, k3, e);
  e = __builtin_fmaf(DP_E4, k4, e);
  e = __builtin_fmaf(DP_E5, k5, e);
  e = __builtin_fmaf(DP_E6, k6, e);
  const float tol = __builtin_fmaf(rtol, fmaxf(fabsf(y), fabsf(y1)), atol);
  return (h * e) / tol;
}

__global__ __launch_bounds__(FLAT_THREADS) void dopri5_finish_kernel(const float* __restrict__ y, const float* __restrict__ k, long ld,
                                                                     const float* __restrict__ h_dev, float atol, float rtol, float* __restrict__ y1,
                                                                     float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const float h = *h_dev;
  float s = 0.f;
  flat_walk(n, true, [&](long v, int cnt, bool whole) {
    float yy[4], a0[4], a2[4], a3[4], a4[4], a5[4], a6[4], o[4];
    flat_load(y, v, cnt, whole, yy);
    flat_load(k, v, cnt, whole, a0);
    flat_load(k + 2 * ld, v, cnt, whole, a2);
    flat_load(k + 3 * ld, v, cnt, whole, a3);
    flat_load(k + 4 * ld, v, cnt, whole, a4);
    flat_load(k + 5 * ld, v, cnt, whole, a5);
    flat_load(k + 6 * ld, v, cnt, whole, a6);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) {
        const float q = finish1(yy[e], a0[e], a2[e], a3[e], a4[e], a5[e], a6[e], h, atol, rtol, o[e]);
        s = __builtin_fmaf(q, q, s);
      }
    flat_store(y1, v, cnt, whole, o);
  });
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------- partial[block] = sum (x / (atol + rtol |y|))^2
__global__ __launch_bounds__(FLAT_THREADS) void rms_norm_scaled_kernel(const float* __restrict__ x, const float* __restrict__ y, float atol, float rtol,
                                                                       float* __restrict__ partial, long n) {
  __shared__ float red[4];
  float s = 0.f;
  flat_walk(n, true, [&](long v, int cnt, bool whole) {
    float xx[4], yy[4];
    flat_load(x, v, cnt, whole, xx);
    flat_load(y, v, cnt, whole, yy);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) {
        const float q = xx[e] / __builtin_fmaf(rtol, fabsf(yy[e]), atol);
        s = __builtin_fmaf(q, q, s);
      }
  });
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------- the quartic through y0, y1, f0, f1 and y_mid, evaluated at t_eval
__device__ __forceinline__ float interp1(float y0, float y1, float ym, float f0, float f1, float h, float x) {
  const float a = 2.f * h * (f1 - f0) - 8.f * (y1 + y0) + 16.f * ym;
  const float b = h * (5.f * f0 - 3.f * f1) + 18.f * y0 + 14.f * y1 - 32.f * ym;
  const float c = h * (f1 - 4.f * f0) - 11.f * y0 - 5.f * y1 + 16.f * ym;
  const float d = h * f0;
  float total = y0 + x * d;
  float xp = x * x;
  total = total + xp * c;
  xp = xp * x;
  total = total + xp * b;
  xp = xp * x;
  return total + xp * a;
}

__global__ __launch_bounds__(FLAT_THREADS) void dopri5_interp_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ ym,
                                                                     const float* __restrict__ k, long ld, const float* __restrict__ h_dev,
                                                                     const float* __restrict__ t0_dev, float t_eval, float* __restrict__ out, long n) {
  // NOT on flat_walk, alone among the walking kernels, and to be left as it stands.  interp1 spells no fma: which of its products are fused is
  // the compiler's choice, and it chooses by the code around them -- the float4 path, the tail loop it unrolls by two and that loop's remainder
  // each round differently (seen in the ISA).  Any other spelling of this loop, the walker's included, moved the bits of the tail elements
  // (tests/test_gpu_flat_bits.py, n % 4 != 0); this one compiles to the instructions it always had (tools/codeobj_diff.py: equal).
  const float h = *h_dev;
  const float x = (t_eval - *t0_dev) / h;
  const float* k6 = k + 6 * ld;
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * FLAT_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < FLAT_UNROLL; ++u) {
    const long v = base + (long)u * FLAT_THREADS;
    if (v < nvec) {
      const float4 a = ((const float4*)y0)[v], b = ((const float4*)y1)[v], m = ((const float4*)ym)[v], f0 = ((const float4*)k)[v],
                   f1 = ((const float4*)k6)[v];
      ((float4*)out)[v] = make_float4(interp1(a.x, b.x, m.x, f0.x, f1.x, h, x), interp1(a.y, b.y, m.y, f0.y, f1.y, h, x),
                                      interp1(a.z, b.z, m.z, f0.z, f1.z, h, x), interp1(a.w, b.w, m.w, f0.w, f1.w, h, x));
    } else if (v == nvec) {
      for (long i = nvec << 2; i < n; ++i) out[i] = interp1(y0[i], y1[i], ym[i], k[i], k6[i], h, x);
    }
  }
}

// ---------------------------------------------------------------- controller (one thread)
__global__ void dopri5_advance_kernel(const float* __restrict__ ratio_dev, float* __restrict__ h_dev, float* __restrict__ t_dev, float* __restrict__ status) {
  const float r = *ratio_dev, h = *h_dev, t = *t_dev;
  const bool accept = r <= 1.f;
  const float dfactor = r < 1.f ? 1.f : 0.2f;                  // an accepted step never shrinks
  const float factor = r == 0.f ? 10.f : fminf(10.f, fmaxf(0.9f / powf(r, 0.2f), dfactor));
  const float t_new = accept ? t + h : t, h_new = h * factor;
  status[0] = accept ? 1.f : 0.f;
  status[1] = r;
  status[2] = t;
  status[3] = h;
  status[4] = t_new;
  status[5] = h_new;
  *t_dev = t_new;
  *h_dev = h_new;
}

// Hairer-Norsett-Wanner starting step.  d = [d0, d1, d2, h0]; phase 0: h0 from d0, d1; phase 1: the step from h0, d1 and d2 = d[2] / h0.
__global__ void dopri5_initial_step_kernel(float* __restrict__ d, int phase, float* __restrict__ h_dev) {
  const float d0 = d[0], d1 = d[1];
  if (phase == 0) {
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    d[3] = h0;
    *h_dev = h0;
  } else {
    const float h0 = d[3], d2 = d[2] / h0;
    const float h1 = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, h0 * 1e-3f) : powf(0.01f / fmaxf(d1, d2), 0.2f);
    *h_dev = fminf(100.f * h0, h1);
  }
}

// ---------------------------------------------------------------- Rademacher probe: Philox4x32-10 (philox_normal.h), one sign per 32-bit word
__device__ __forceinline__ float rad_sign(unsigned w) { return (w >> 31) ? 1.f : -1.f; }      // the top bit of the word

// item v = the four signs of elements 4 v .. 4 v + 3 = the four words of the block with counter (counter, v); vec: out is 16-byte aligned
__global__ __launch_bounds__(FLAT_THREADS) void rademacher_kernel(float* __restrict__ out, long n, PhiloxWords w, int vec) {
  flat_walk(n, vec, [&](long v, int cnt, bool whole) {
    unsigned c[4] = {w.c0, w.c1, (unsigned)((unsigned long)v & 0xffffffffu), (unsigned)((unsigned long)v >> 32)};
    philox4x32_10(c, w.k0, w.k1);
    const float s[4] = {rad_sign(c[0]), rad_sign(c[1]), rad_sign(c[2]), rad_sign(c[3])};
    flat_store(out, v, cnt, whole, s);
  });
}

// ---------------------------------------------------------------- out[r] = sum_j a[r, j] b[r, j], rows of m floats
// row_reduce of flat_common.h with one fma per element and the sum itself as the result
struct DotTerm {
  __device__ float operator()(float a, float b, float s) const { return __builtin_fmaf(a, b, s); }
};
struct SumFinish {
  __device__ float operator()(float s) const { return s; }
};

// logp[b] = (c - sumsq[b] / 2) - delta[b], each operation rounded once (no contraction: the host formula, operation by operation)
__global__ void likelihood_finish_kernel(const float* __restrict__ sumsq, const float* __restrict__ delta, float c, float* __restrict__ logp, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) logp[i] = __fsub_rn(__fsub_rn(c, __fmul_rn(sumsq[i], 0.5f)), delta[i]);
}

// ---------------------------------------------------------------- SDE sampler: the standard-normal draw and the step's linear combination
// The draw itself (Philox block -> Box-Muller -> four normals) is philox_normal4 of philox_normal.h.
__global__ __launch_bounds__(FLAT_THREADS) void normal_kernel(float* __restrict__ out, long n, PhiloxWords w, int vec) {
  flat_walk(n, vec, [&](long v, int cnt, bool whole) {
    float z[4];
    philox_normal4(v, w.k0, w.k1, w.c0, w.c1, z);
    flat_store(out, v, cnt, whole, z);
  });
}

// out = sum_{j < M} coef_j in_j (+ noise_coef z); mean_out (optional) = the sum without the noise term.  NOISE 0: none, 1: z read from memory,
// 2: z drawn here (philox_normal4) and never stored.  out / mean_out may BE one of the inputs (an item is read whole before it is written, and
// no other thread touches it), hence no __restrict__ on them or on the inputs.
struct SdeIn { const float* p[4]; float c[4]; };
enum { SDE_NOISE_NONE = 0, SDE_NOISE_TENSOR = 1, SDE_NOISE_PHILOX = 2 };

template <int M> __device__ __forceinline__ float sde_sum(const float (&x)[4], const SdeIn& a) {
  float acc = __fmul_rn(a.c[0], x[0]);
#pragma unroll
  for (int j = 1; j < M; ++j) acc = __builtin_fmaf(a.c[j], x[j], acc);
  return acc;
}

template <int M, int NOISE>
__global__ __launch_bounds__(FLAT_THREADS) void sde_combine_kernel(SdeIn a, const float* zt, float noise_coef, PhiloxWords w, float* out, float* mean_out,
                                                                   long n, float t_next, float* __restrict__ t_out, int nt) {
  flat_fill_side(t_out, nt, t_next);                            // the time vector of the NEXT model evaluation, one value per sample
  flat_walk(n, true, [&](long v, int cnt, bool whole) {
    float z[4] = {0.f, 0.f, 0.f, 0.f}, x[M][4], m[4], o[4];
    if (NOISE == SDE_NOISE_PHILOX) philox_normal4(v, w.k0, w.k1, w.c0, w.c1, z);
    if (NOISE == SDE_NOISE_TENSOR) flat_load(zt, v, cnt, whole, z);
#pragma unroll
    for (int j = 0; j < M; ++j) flat_load(a.p[j], v, cnt, whole, x[j]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xe[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < M; ++j) xe[j] = x[j][e];
      m[e] = sde_sum<M>(xe, a);
      o[e] = NOISE == SDE_NOISE_NONE ? m[e] : __builtin_fmaf(noise_coef, z[e], m[e]);
    }
    if (mean_out) flat_store(mean_out, v, cnt, whole, m);
    flat_store(out, v, cnt, whole, o);
  });
}

template <int M>
void launch_sde_combine(int noise, const SdeIn& a, const float* z, float noise_coef, PhiloxWords w, float* out, float* mean_out, long n, float t_next,
                        float* t_out, int nt, hipStream_t st) {
  const dim3 grid(ode_grid(n)), block(FLAT_THREADS);
  if (noise == SDE_NOISE_NONE)
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_NONE>), grid, block, 0, st, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt);
  else if (noise == SDE_NOISE_TENSOR)
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_TENSOR>), grid, block, 0, st, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt);
  else
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_PHILOX>), grid, block, 0, st, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt);
}

template <int M>
void launch_stage(const float* y, const float* k, long ld, const RkCoef& cf, const float* h_dev, float* out, long n, const float* t_dev, float ct,
                  float* t_out, int nt, hipStream_t st) {
  hipLaunchKernelGGL(rk_stage_kernel<M>, dim3(ode_grid(n)), dim3(FLAT_THREADS), 0, st, y, k, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt);
}

}  // namespace

extern "C" int ldmae_ode_partials(long n) { return n > 0 ? (int)ode_grid(n) : 0; }

extern "C" int ldmae_rk_stage_f32(const float* y, const float* k_slab, long ld, const float* coef, int m, const float* h_dev, float* out, long n,
                                  const float* t_dev, float ct, float* t_out, int nt, void* stream) {
  LDMAE_REQUIRE(y && k_slab && coef && h_dev && out && n > 0 && m >= 1 && m <= 7, "rk_stage: bad arguments (m = %d, n = %ld)", m, n);
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && is_aligned(y) && is_aligned(k_slab) && is_aligned(out), "rk_stage: ld %ld must be a multiple of 4, >= n, and y, k_slab, out 16-byte aligned", ld);
  LDMAE_REQUIRE(!t_out || (t_dev && nt > 0), "rk_stage: t_out needs t_dev and nt > 0");
  LDMAE_REQUIRE(flat_fits_grid(n), "rk_stage: n too large");
  RkCoef cf;
  for (int j = 0; j < 7; ++j) cf.c[j] = j < m ? coef[j] : 0.f;
  hipStream_t st = as_stream(stream);
  switch (m) {
    case 1: launch_stage<1>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    case 2: launch_stage<2>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    case 3: launch_stage<3>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    case 4: launch_stage<4>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    case 5: launch_stage<5>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    case 6: launch_stage<6>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
    default: launch_stage<7>(y, k_slab, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt, st); break;
  }
  LDMAE_CHECK_LAUNCH("rk_stage");
  return LDMAE_OK;
}

extern "C" int ldmae_dopri5_finish_f32(const float* y, const float* k_slab, long ld, const float* h_dev, float atol, float rtol, float* y1,
                                       float* partial, float* ratio_dev, long n, void* stream) {
  LDMAE_REQUIRE(y && k_slab && h_dev && y1 && partial && ratio_dev && n > 0, "dopri5_finish: bad arguments");
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && is_aligned(y) && is_aligned(k_slab) && is_aligned(y1), "dopri5_finish: ld %ld must be a multiple of 4, >= n, and y, k_slab, y1 16-byte aligned", ld);
  LDMAE_REQUIRE(y1 != y, "dopri5_finish: y1 must not alias y");
  const unsigned grid = ode_grid(n);
  hipLaunchKernelGGL(dopri5_finish_kernel, dim3(grid), dim3(FLAT_THREADS), 0, as_stream(stream), y, k_slab, ld, h_dev, atol, rtol, y1, partial, n);
  launch_rms_fold(partial, grid, n, ratio_dev, as_stream(stream));
  LDMAE_CHECK_LAUNCH("dopri5_finish");
  return LDMAE_OK;
}

extern "C" int ldmae_rms_norm_scaled_f32(const float* x, const float* y_or_null, float atol, float rtol, float* partial, float* out_dev, long n,
                                         void* stream) {
  LDMAE_REQUIRE(x && partial && out_dev && n > 0, "rms_norm_scaled: bad arguments");
  const float* y = y_or_null ? y_or_null : x;
  LDMAE_REQUIRE(is_aligned(x) && is_aligned(y), "rms_norm_scaled: x and y must be 16-byte aligned");
  const unsigned grid = ode_grid(n);
  hipLaunchKernelGGL(rms_norm_scaled_kernel, dim3(grid), dim3(FLAT_THREADS), 0, as_stream(stream), x, y, atol, rtol, partial, n);
  launch_rms_fold(partial, grid, n, out_dev, as_stream(stream));
  LDMAE_CHECK_LAUNCH("rms_norm_scaled");
  return LDMAE_OK;
}

extern "C" int ldmae_dopri5_interp_f32(const float* y0, const float* y1, const float* y_mid, const float* k_slab, long ld, const float* h_dev,
                                       const float* t0_dev, float t_eval, float* out, long n, void* stream) {
  LDMAE_REQUIRE(y0 && y1 && y_mid && k_slab && h_dev && t0_dev && out && n > 0, "dopri5_interp: bad arguments");
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && is_aligned(y0) && is_aligned(y1) && is_aligned(y_mid) && is_aligned(k_slab) && is_aligned(out),
                "dopri5_interp: ld %ld must be a multiple of 4, >= n, and every tensor 16-byte aligned", ld);
  hipLaunchKernelGGL(dopri5_interp_kernel, dim3(ode_grid(n)), dim3(FLAT_THREADS), 0, as_stream(stream), y0, y1, y_mid, k_slab, ld, h_dev, t0_dev, t_eval,
                     out, n);
  LDMAE_CHECK_LAUNCH("dopri5_interp");
  return LDMAE_OK;
}

extern "C" int ldmae_dopri5_advance(const float* ratio_dev, float* h_dev, float* t_dev, float* status_dev, void* stream) {
  LDMAE_REQUIRE(ratio_dev && h_dev && t_dev && status_dev, "dopri5_advance: bad arguments");
  hipLaunchKernelGGL(dopri5_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), ratio_dev, h_dev, t_dev, status_dev);
  LDMAE_CHECK_LAUNCH("dopri5_advance");
  return LDMAE_OK;
}

extern "C" int ldmae_dopri5_initial_step(float* d_dev, int phase, float* h_dev, void* stream) {
  LDMAE_REQUIRE(d_dev && h_dev && (phase == 0 || phase == 1), "dopri5_initial_step: bad arguments");
  hipLaunchKernelGGL(dopri5_initial_step_kernel, dim3(1), dim3(1), 0, as_stream(stream), d_dev, phase, h_dev);
  LDMAE_CHECK_LAUNCH("dopri5_initial_step");
  return LDMAE_OK;
}

extern "C" int ldmae_rademacher_f32(float* out, long n, unsigned long long seed, unsigned long long counter, void* stream) {
  LDMAE_REQUIRE(out && n > 0 && ((uintptr_t)out & 3) == 0, "rademacher: bad arguments (n = %ld)", n);
  LDMAE_REQUIRE(flat_fits_grid(n), "rademacher: n too large");
  hipLaunchKernelGGL(rademacher_kernel, dim3(ode_grid(n)), dim3(FLAT_THREADS), 0, as_stream(stream), out, n, PhiloxWords(seed, counter),
                     is_aligned(out) ? 1 : 0);
  LDMAE_CHECK_LAUNCH("rademacher");
  return LDMAE_OK;
}

extern "C" int ldmae_normal_f32(float* out, long n, unsigned long long seed, unsigned long long counter, void* stream) {
  LDMAE_REQUIRE(out && n > 0 && ((uintptr_t)out & 3) == 0, "normal: bad arguments (n = %ld)", n);
  LDMAE_REQUIRE(flat_fits_grid(n), "normal: n too large");
  hipLaunchKernelGGL(normal_kernel, dim3(ode_grid(n)), dim3(FLAT_THREADS), 0, as_stream(stream), out, n, PhiloxWords(seed, counter),
                     is_aligned(out) ? 1 : 0);
  LDMAE_CHECK_LAUNCH("normal");
  return LDMAE_OK;
}

extern "C" int ldmae_sde_combine_f32(const float* in0, const float* in1, const float* in2, const float* in3, const float* coef, int m, const float* z,
                                     float noise_coef, int noise_mode, unsigned long long seed, unsigned long long counter, float* out,
                                     float* mean_out, long n, float t_next, float* t_out, int nt, void* stream) {
  LDMAE_REQUIRE(coef && out && n > 0 && m >= 1 && m <= 4, "sde_combine: bad arguments (m = %d, n = %ld)", m, n);
  LDMAE_REQUIRE(noise_mode >= SDE_NOISE_NONE && noise_mode <= SDE_NOISE_PHILOX, "sde_combine: noise_mode %d (0 none, 1 tensor, 2 Philox)", noise_mode);
  LDMAE_REQUIRE((noise_mode == SDE_NOISE_TENSOR) == (z != nullptr), "sde_combine: z is given exactly when noise_mode is 1");
  LDMAE_REQUIRE(!t_out || (nt > 0 && ((uintptr_t)t_out & 3) == 0), "sde_combine: t_out needs nt > 0 and 4-byte alignment");
  LDMAE_REQUIRE(flat_fits_grid(n), "sde_combine: n too large");
  SdeIn a;
  const float* in[4] = {in0, in1, in2, in3};
  for (int j = 0; j < 4; ++j) {
    a.p[j] = j < m ? in[j] : nullptr;
    a.c[j] = j < m ? coef[j] : 0.f;
    LDMAE_REQUIRE(j >= m || (in[j] && is_aligned(in[j])), "sde_combine: input %d is null or not 16-byte aligned", j);
  }
  LDMAE_REQUIRE(is_aligned(out) && is_aligned(mean_out) && is_aligned(z), "sde_combine: out, mean_out and z must be 16-byte aligned");
  // in place is allowed (out or mean_out IS an input); a partial overlap would let one thread read what another has already written
  LDMAE_REQUIRE(!mean_out || (mean_out + n <= out || out + n <= mean_out), "sde_combine: out and mean_out overlap");
  for (int j = 0; j < m; ++j)
    LDMAE_REQUIRE(same_or_disjoint(out, in[j], n) && (!mean_out || same_or_disjoint(mean_out, in[j], n)),
                  "sde_combine: an output partially overlaps input %d (in place means the same pointer)", j);
  LDMAE_REQUIRE(!z || (same_or_disjoint(out, z, n) && (!mean_out || same_or_disjoint(mean_out, z, n))), "sde_combine: an output partially overlaps z");
  if (t_out) {
    const float* all[7] = {in0, in1, in2, in3, z, out, mean_out};
    for (int j = 0; j < 7; ++j)
      LDMAE_REQUIRE(!all[j] || (j < 4 && j >= m) || t_out + nt <= all[j] || all[j] + n <= t_out, "sde_combine: t_out overlaps a tensor of the step");
  }
  hipStream_t st = as_stream(stream);
  const PhiloxWords w(seed, counter);
  switch (m) {
    case 1: launch_sde_combine<1>(noise_mode, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt, st); break;
    case 2: launch_sde_combine<2>(noise_mode, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt, st); break;
    case 3: launch_sde_combine<3>(noise_mode, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt, st); break;
    default: launch_sde_combine<4>(noise_mode, a, z, noise_coef, w, out, mean_out, n, t_next, t_out, nt, st); break;
  }
  LDMAE_CHECK_LAUNCH("sde_combine");
  return LDMAE_OK;
}

extern "C" long ldmae_rowdot_partials(int B, long m) { return row_partials(B, m); }

extern "C" int ldmae_rowdot_f32(const float* a, const float* b, float* out, int B, long m, float* partial, void* stream) {
  LDMAE_REQUIRE(a && b && out && partial && B > 0 && m > 0, "rowdot: bad arguments (B = %d, m = %ld)", B, m);
  LDMAE_REQUIRE(is_aligned(a, 4) && is_aligned(b, 4), "rowdot: a and b must be 4-byte aligned");
  LDMAE_REQUIRE(row_fits_grid(B, m), "rowdot: B * ceil(m / 4096) = %ld blocks is too many", (long)B * row_chunks(m));
  row_reduce<DotTerm>(a, b, out, B, m, partial, row_vec(is_aligned(a), is_aligned(b), B, m), SumFinish{}, as_stream(stream));
  LDMAE_CHECK_LAUNCH("rowdot");
  return LDMAE_OK;
}

extern "C" int ldmae_likelihood_finish_f32(const float* sumsq, const float* delta, float c, float* logp, int B, void* stream) {
  LDMAE_REQUIRE(sumsq && delta && logp && B > 0, "likelihood_finish: bad arguments");
  hipLaunchKernelGGL(likelihood_finish_kernel, dim3(cdiv(B, 256)), dim3(256), 0, as_stream(stream), sumsq, delta, c, logp, B);
  LDMAE_CHECK_LAUNCH("likelihood_finish");
  return LDMAE_OK;
}
