// Adaptive Dormand-Prince 5(4) ODE sampler (transport/integrators.py, sampler_type "dopri5"): the solver's own arithmetic between two model
// evaluations.  All f32, plain vector code, every kernel bound by HBM traffic (one pass over its operands, 16-byte accesses).
//
// Layout.  The seven stage derivatives live in one slab k[7][ld] (ld % 4 == 0, ld >= n: every row 16-byte aligned for any n).  A kernel
// walks "items": item v < n / 4 is the float4 at element 4 v, item n / 4 (present when n % 4 != 0) is the scalar tail.  A block of 256 threads
// owns 1024 consecutive items, thread t the items t, t + 256, t + 512, t + 768 of them, so the grid is cdiv(items, 1024): a function of n
// alone, never of the device.
//
// Reductions (the error ratio and the norms of the initial-step rule) are two-stage and fixed-order, no atomics: a thread adds its (up to 16)
// squares in element order, a wave joins its 64 lanes in the xor butterfly 32, 16, 8, 4, 2, 1, the four waves are added as (w0 + w1) + (w2 + w3)
// and the block stores partial[block].  ode_fold_kernel (one block) lets thread t add partial[t], partial[t + 256], ... in that order, joins
// the 256 threads the same way and writes sqrt(sum / n).  The order depends on n only: two runs give the same bits.
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
#include "common.h"
#include "philox_normal.h"

namespace {

constexpr int ODE_THREADS = 256;
constexpr int ODE_UNROLL = 4;                                   // items per thread
constexpr long ODE_BLOCK_ITEMS = (long)ODE_THREADS * ODE_UNROLL;

struct RkCoef { float c[7]; };

// c_sol (= row 7 of the tableau: FSAL), c_error = c_sol - the embedded 4th-order weights; b[1] = e[1] = 0 and b[6] = 0
constexpr float DP_B0 = (float)(35.0 / 384.0), DP_B2 = (float)(500.0 / 1113.0), DP_B3 = (float)(125.0 / 192.0), DP_B4 = (float)(-2187.0 / 6784.0),
                DP_B5 = (float)(11.0 / 84.0);
constexpr float DP_E0 = (float)(35.0 / 384.0 - 1951.0 / 21600.0), DP_E2 = (float)(500.0 / 1113.0 - 22642.0 / 50085.0),
                DP_E3 = (float)(125.0 / 192.0 - 451.0 / 720.0), DP_E4 = (float)(-2187.0 / 6784.0 + 12231.0 / 42400.0),
                DP_E5 = (float)(11.0 / 84.0 - 649.0 / 6300.0), DP_E6 = (float)(-1.0 / 60.0);

inline long ode_items(long n) { return (n >> 2) + ((n & 3) ? 1 : 0); }
inline unsigned ode_grid(long n) { return cdiv(ode_items(n), ODE_BLOCK_ITEMS); }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------- out = y + h * sum_{j < M} coef_j k_j
template <int M> __device__ __forceinline__ float stage1(float y, const float (&k)[7], const RkCoef& cf, float h) {
  float acc = cf.c[0] * k[0];
#pragma unroll
  for (int j = 1; j < M; ++j) acc = __builtin_fmaf(cf.c[j], k[j], acc);
  return __builtin_fmaf(h, acc, y);
}

template <int M>
__global__ __launch_bounds__(ODE_THREADS) void rk_stage_kernel(const float* __restrict__ y, const float* __restrict__ k, long ld, RkCoef cf,
                                                               const float* __restrict__ h_dev, float* out, long n,
                                                               const float* __restrict__ t_dev, float ct, float* __restrict__ t_out, int nt) {
  const float h = *h_dev;
  if (t_out && blockIdx.x == 0) {                               // the time the NEXT model evaluation is fed: t + ct h, one value per sample
    const float ts = __builtin_fmaf(ct, h, *t_dev);
    for (int i = threadIdx.x; i < nt; i += ODE_THREADS) t_out[i] = ts;
  }
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v < nvec) {
      const float4 yy = ((const float4*)y)[v];
      float4 kk[M];
#pragma unroll
      for (int j = 0; j < M; ++j) kk[j] = ((const float4*)(k + (long)j * ld))[v];
      float a[7], b[7], c[7], d[7];
#pragma unroll
      for (int j = 0; j < M; ++j) { a[j] = kk[j].x; b[j] = kk[j].y; c[j] = kk[j].z; d[j] = kk[j].w; }
      ((float4*)out)[v] = make_float4(stage1<M>(yy.x, a, cf, h), stage1<M>(yy.y, b, cf, h), stage1<M>(yy.z, c, cf, h), stage1<M>(yy.w, d, cf, h));
    } else if (v == nvec) {
      for (long i = nvec << 2; i < n; ++i) {
        float kj[7];
#pragma unroll
        for (int j = 0; j < M; ++j) kj[j] = k[(long)j * ld + i];
        out[i] = stage1<M>(y[i], kj, cf, h);
      }
    }
  }
}

// ---------------------------------------------------------------- block sum (fixed order), see the header comment
__device__ __forceinline__ float ode_block_sum(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(ODE_THREADS) void ode_fold_kernel(const float* __restrict__ partial, int nparts, float n, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += ODE_THREADS) s += partial[i];
  s = ode_block_sum(s, red);
  if (threadIdx.x == 0) *out = sqrtf(s / n);
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

__global__ __launch_bounds__(ODE_THREADS) void dopri5_finish_kernel(const float* __restrict__ y, const float* __restrict__ k, long ld,
                                                                    const float* __restrict__ h_dev, float atol, float rtol, float* __restrict__ y1,
                                                                    float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const float h = *h_dev;
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
  const float *k2 = k + 2 * ld, *k3 = k + 3 * ld, *k4 = k + 4 * ld, *k5 = k + 5 * ld, *k6 = k + 6 * ld;
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v < nvec) {
      const float4 yy = ((const float4*)y)[v], a0 = ((const float4*)k)[v], a2 = ((const float4*)k2)[v], a3 = ((const float4*)k3)[v],
                   a4 = ((const float4*)k4)[v], a5 = ((const float4*)k5)[v], a6 = ((const float4*)k6)[v];
      float4 o;
      float q;
      q = finish1(yy.x, a0.x, a2.x, a3.x, a4.x, a5.x, a6.x, h, atol, rtol, o.x); s = __builtin_fmaf(q, q, s);
      q = finish1(yy.y, a0.y, a2.y, a3.y, a4.y, a5.y, a6.y, h, atol, rtol, o.y); s = __builtin_fmaf(q, q, s);
      q = finish1(yy.z, a0.z, a2.z, a3.z, a4.z, a5.z, a6.z, h, atol, rtol, o.z); s = __builtin_fmaf(q, q, s);
      q = finish1(yy.w, a0.w, a2.w, a3.w, a4.w, a5.w, a6.w, h, atol, rtol, o.w); s = __builtin_fmaf(q, q, s);
      ((float4*)y1)[v] = o;
    } else if (v == nvec) {
      for (long i = nvec << 2; i < n; ++i) {
        float o;
        const float q = finish1(y[i], k[i], k2[i], k3[i], k4[i], k5[i], k6[i], h, atol, rtol, o);
        s = __builtin_fmaf(q, q, s);
        y1[i] = o;
      }
    }
  }
  s = ode_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------- partial[block] = sum (x / (atol + rtol |y|))^2
__global__ __launch_bounds__(ODE_THREADS) void rms_norm_scaled_kernel(const float* __restrict__ x, const float* __restrict__ y, float atol, float rtol,
                                                                      float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v < nvec) {
      const float4 xx = ((const float4*)x)[v], yy = ((const float4*)y)[v];
      float q;
      q = xx.x / __builtin_fmaf(rtol, fabsf(yy.x), atol); s = __builtin_fmaf(q, q, s);
      q = xx.y / __builtin_fmaf(rtol, fabsf(yy.y), atol); s = __builtin_fmaf(q, q, s);
      q = xx.z / __builtin_fmaf(rtol, fabsf(yy.z), atol); s = __builtin_fmaf(q, q, s);
      q = xx.w / __builtin_fmaf(rtol, fabsf(yy.w), atol); s = __builtin_fmaf(q, q, s);
    } else if (v == nvec) {
      for (long i = nvec << 2; i < n; ++i) {
        const float q = x[i] / __builtin_fmaf(rtol, fabsf(y[i]), atol);
        s = __builtin_fmaf(q, q, s);
      }
    }
  }
  s = ode_block_sum(s, red);
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

__global__ __launch_bounds__(ODE_THREADS) void dopri5_interp_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ ym,
                                                                    const float* __restrict__ k, long ld, const float* __restrict__ h_dev,
                                                                    const float* __restrict__ t0_dev, float t_eval, float* __restrict__ out, long n) {
  const float h = *h_dev;
  const float x = (t_eval - *t0_dev) / h;
  const float* k6 = k + 6 * ld;
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
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
__global__ __launch_bounds__(ODE_THREADS) void rademacher_kernel(float* __restrict__ out, long n, unsigned k0, unsigned k1, unsigned c0, unsigned c1,
                                                                 int vec) {
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v > nvec || (v == nvec && (n & 3) == 0)) continue;
    unsigned c[4] = {c0, c1, (unsigned)((unsigned long)v & 0xffffffffu), (unsigned)((unsigned long)v >> 32)};
    philox4x32_10(c, k0, k1);
    const float s[4] = {rad_sign(c[0]), rad_sign(c[1]), rad_sign(c[2]), rad_sign(c[3])};
    if (v < nvec && vec) {
      ((float4*)out)[v] = make_float4(s[0], s[1], s[2], s[3]);
    } else {
      const long e0 = v << 2;
      for (int j = 0; j < 4; ++j)
        if (e0 + j < n) out[e0 + j] = s[j];
    }
  }
}

// ---------------------------------------------------------------- out[r] = sum_j a[r, j] b[r, j], rows of m floats
// Stage 1: block (r, c) owns the 4096 elements [4096 c, 4096 c + 4096) of row r.  vec (both row starts 16-byte aligned for every r): thread t
// takes the float4s t, t + 256, t + 512, t + 768 of the chunk, element order inside each; otherwise thread t takes the elements t, t + 256, ...
// (16 of them).  One fma chain per thread, then ode_block_sum; partial[r * chunks + c].  Stage 2: one block per row folds its chunks.
constexpr long ROW_CHUNK = 4096;

__global__ __launch_bounds__(ODE_THREADS) void rowdot_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ partial,
                                                             long m, long chunks, int vec) {
  __shared__ float red[4];
  const long r = blockIdx.x / chunks, c = blockIdx.x - r * chunks;
  const float *ar = a + r * m, *br = b + r * m;
  const long lo = c * ROW_CHUNK, hi = lo + ROW_CHUNK < m ? lo + ROW_CHUNK : m;
  float s = 0.f;
  if (vec) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long e = lo + 4 * ((long)threadIdx.x + (long)u * ODE_THREADS);
      if (e + 4 <= hi) {
        const float4 x = *(const float4*)(ar + e), y = *(const float4*)(br + e);
        s = __builtin_fmaf(x.x, y.x, s); s = __builtin_fmaf(x.y, y.y, s); s = __builtin_fmaf(x.z, y.z, s); s = __builtin_fmaf(x.w, y.w, s);
      } else {
        for (long i = e; i < hi; ++i) s = __builtin_fmaf(ar[i], br[i], s);
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const long i = lo + threadIdx.x + (long)u * ODE_THREADS;
      if (i < hi) s = __builtin_fmaf(ar[i], br[i], s);
    }
  }
  s = ode_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(ODE_THREADS) void rowdot_fold_kernel(const float* __restrict__ partial, long chunks, float* __restrict__ out) {
  __shared__ float red[4];
  const float* p = partial + (long)blockIdx.x * chunks;
  float s = 0.f;
  for (long i = threadIdx.x; i < chunks; i += ODE_THREADS) s += p[i];
  s = ode_block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// logp[b] = (c - sumsq[b] / 2) - delta[b], each operation rounded once (no contraction: the host formula, operation by operation)
__global__ void likelihood_finish_kernel(const float* __restrict__ sumsq, const float* __restrict__ delta, float c, float* __restrict__ logp, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) logp[i] = __fsub_rn(__fsub_rn(c, __fmul_rn(sumsq[i], 0.5f)), delta[i]);
}

// ---------------------------------------------------------------- SDE sampler: the standard-normal draw and the step's linear combination
// The draw itself (Philox block -> Box-Muller -> four normals) is philox_normal4 of philox_normal.h.
__global__ __launch_bounds__(ODE_THREADS) void normal_kernel(float* __restrict__ out, long n, unsigned k0, unsigned k1, unsigned c0, unsigned c1, int vec) {
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v > nvec || (v == nvec && (n & 3) == 0)) continue;
    float z[4];
    philox_normal4(v, k0, k1, c0, c1, z);
    if (v < nvec && vec) {
      ((float4*)out)[v] = make_float4(z[0], z[1], z[2], z[3]);
    } else {
      const long e0 = v << 2;
      for (int j = 0; j < 4; ++j)
        if (e0 + j < n) out[e0 + j] = z[j];
    }
  }
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
__global__ __launch_bounds__(ODE_THREADS) void sde_combine_kernel(SdeIn a, const float* zt, float noise_coef, unsigned k0, unsigned k1, unsigned c0,
                                                                  unsigned c1, float* out, float* mean_out, long n, float t_next,
                                                                  float* __restrict__ t_out, int nt) {
  if (t_out && blockIdx.x == 0)                                 // the time vector of the NEXT model evaluation, one value per sample
    for (int i = threadIdx.x; i < nt; i += ODE_THREADS) t_out[i] = t_next;
  const long nvec = n >> 2;
  const long base = (long)blockIdx.x * ODE_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < ODE_UNROLL; ++u) {
    const long v = base + (long)u * ODE_THREADS;
    if (v > nvec || (v == nvec && (n & 3) == 0)) continue;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (NOISE == SDE_NOISE_PHILOX) philox_normal4(v, k0, k1, c0, c1, z);
    if (v < nvec) {
      float4 x[M];
#pragma unroll
      for (int j = 0; j < M; ++j) x[j] = ((const float4*)a.p[j])[v];
      if (NOISE == SDE_NOISE_TENSOR) {
        const float4 zz = ((const float4*)zt)[v];
        z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
      }
      float xa[4] = {0.f, 0.f, 0.f, 0.f}, xb[4] = {0.f, 0.f, 0.f, 0.f}, xc[4] = {0.f, 0.f, 0.f, 0.f}, xd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < M; ++j) { xa[j] = x[j].x; xb[j] = x[j].y; xc[j] = x[j].z; xd[j] = x[j].w; }
      const float4 m = make_float4(sde_sum<M>(xa, a), sde_sum<M>(xb, a), sde_sum<M>(xc, a), sde_sum<M>(xd, a));
      if (mean_out) ((float4*)mean_out)[v] = m;
      ((float4*)out)[v] = NOISE == SDE_NOISE_NONE ? m : make_float4(__builtin_fmaf(noise_coef, z[0], m.x), __builtin_fmaf(noise_coef, z[1], m.y),
                                                                    __builtin_fmaf(noise_coef, z[2], m.z), __builtin_fmaf(noise_coef, z[3], m.w));
    } else {
      const long e0 = nvec << 2;
      for (int e = 0; e < 4; ++e) {
        const long i = e0 + e;
        if (i >= n) break;
        float xi[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < M; ++j) xi[j] = a.p[j][i];
        const float zi = NOISE == SDE_NOISE_TENSOR ? zt[i] : z[e];
        const float m = sde_sum<M>(xi, a);
        if (mean_out) mean_out[i] = m;
        out[i] = NOISE == SDE_NOISE_NONE ? m : __builtin_fmaf(noise_coef, zi, m);
      }
    }
  }
}

template <int M>
void launch_sde_combine(int noise, const SdeIn& a, const float* z, float noise_coef, unsigned long long seed, unsigned long long counter, float* out,
                        float* mean_out, long n, float t_next, float* t_out, int nt, hipStream_t st) {
  const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32), c0 = (unsigned)(counter & 0xffffffffu), c1 = (unsigned)(counter >> 32);
  const dim3 grid(ode_grid(n)), block(ODE_THREADS);
  if (noise == SDE_NOISE_NONE)
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_NONE>), grid, block, 0, st, a, z, noise_coef, k0, k1, c0, c1, out, mean_out, n, t_next, t_out, nt);
  else if (noise == SDE_NOISE_TENSOR)
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_TENSOR>), grid, block, 0, st, a, z, noise_coef, k0, k1, c0, c1, out, mean_out, n, t_next, t_out, nt);
  else
    hipLaunchKernelGGL((sde_combine_kernel<M, SDE_NOISE_PHILOX>), grid, block, 0, st, a, z, noise_coef, k0, k1, c0, c1, out, mean_out, n, t_next, t_out, nt);
}

// [a, a + n) and [b, b + n) floats: identical or disjoint
inline bool same_or_disjoint(const float* a, const float* b, long n) { return a == b || a + n <= b || b + n <= a; }

template <int M>
void launch_stage(const float* y, const float* k, long ld, const RkCoef& cf, const float* h_dev, float* out, long n, const float* t_dev, float ct,
                  float* t_out, int nt, hipStream_t st) {
  hipLaunchKernelGGL(rk_stage_kernel<M>, dim3(ode_grid(n)), dim3(ODE_THREADS), 0, st, y, k, ld, cf, h_dev, out, n, t_dev, ct, t_out, nt);
}

}  // namespace

extern "C" int ldmae_ode_partials(long n) { return n > 0 ? (int)ode_grid(n) : 0; }

extern "C" int ldmae_rk_stage_f32(const float* y, const float* k_slab, long ld, const float* coef, int m, const float* h_dev, float* out, long n,
                                  const float* t_dev, float ct, float* t_out, int nt, void* stream) {
  LDMAE_REQUIRE(y && k_slab && coef && h_dev && out && n > 0 && m >= 1 && m <= 7, "rk_stage: bad arguments (m = %d, n = %ld)", m, n);
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && al16(y) && al16(k_slab) && al16(out), "rk_stage: ld %ld must be a multiple of 4, >= n, and y, k_slab, out 16-byte aligned", ld);
  LDMAE_REQUIRE(!t_out || (t_dev && nt > 0), "rk_stage: t_out needs t_dev and nt > 0");
  LDMAE_REQUIRE(ode_items(n) <= 0x7fffffffL * ODE_BLOCK_ITEMS, "rk_stage: n too large");
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
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && al16(y) && al16(k_slab) && al16(y1), "dopri5_finish: ld %ld must be a multiple of 4, >= n, and y, k_slab, y1 16-byte aligned", ld);
  LDMAE_REQUIRE(y1 != y, "dopri5_finish: y1 must not alias y");
  const unsigned grid = ode_grid(n);
  hipLaunchKernelGGL(dopri5_finish_kernel, dim3(grid), dim3(ODE_THREADS), 0, as_stream(stream), y, k_slab, ld, h_dev, atol, rtol, y1, partial, n);
  hipLaunchKernelGGL(ode_fold_kernel, dim3(1), dim3(ODE_THREADS), 0, as_stream(stream), partial, (int)grid, (float)n, ratio_dev);
  LDMAE_CHECK_LAUNCH("dopri5_finish");
  return LDMAE_OK;
}

extern "C" int ldmae_rms_norm_scaled_f32(const float* x, const float* y_or_null, float atol, float rtol, float* partial, float* out_dev, long n,
                                         void* stream) {
  LDMAE_REQUIRE(x && partial && out_dev && n > 0, "rms_norm_scaled: bad arguments");
  const float* y = y_or_null ? y_or_null : x;
  LDMAE_REQUIRE(al16(x) && al16(y), "rms_norm_scaled: x and y must be 16-byte aligned");
  const unsigned grid = ode_grid(n);
  hipLaunchKernelGGL(rms_norm_scaled_kernel, dim3(grid), dim3(ODE_THREADS), 0, as_stream(stream), x, y, atol, rtol, partial, n);
  hipLaunchKernelGGL(ode_fold_kernel, dim3(1), dim3(ODE_THREADS), 0, as_stream(stream), partial, (int)grid, (float)n, out_dev);
  LDMAE_CHECK_LAUNCH("rms_norm_scaled");
  return LDMAE_OK;
}

extern "C" int ldmae_dopri5_interp_f32(const float* y0, const float* y1, const float* y_mid, const float* k_slab, long ld, const float* h_dev,
                                       const float* t0_dev, float t_eval, float* out, long n, void* stream) {
  LDMAE_REQUIRE(y0 && y1 && y_mid && k_slab && h_dev && t0_dev && out && n > 0, "dopri5_interp: bad arguments");
  LDMAE_REQUIRE(ld >= n && (ld & 3) == 0 && al16(y0) && al16(y1) && al16(y_mid) && al16(k_slab) && al16(out),
                "dopri5_interp: ld %ld must be a multiple of 4, >= n, and every tensor 16-byte aligned", ld);
  hipLaunchKernelGGL(dopri5_interp_kernel, dim3(ode_grid(n)), dim3(ODE_THREADS), 0, as_stream(stream), y0, y1, y_mid, k_slab, ld, h_dev, t0_dev, t_eval,
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
  LDMAE_REQUIRE(ode_items(n) <= 0x7fffffffL * ODE_BLOCK_ITEMS, "rademacher: n too large");
  hipLaunchKernelGGL(rademacher_kernel, dim3(ode_grid(n)), dim3(ODE_THREADS), 0, as_stream(stream), out, n, (unsigned)(seed & 0xffffffffu),
                     (unsigned)(seed >> 32), (unsigned)(counter & 0xffffffffu), (unsigned)(counter >> 32), al16(out) ? 1 : 0);
  LDMAE_CHECK_LAUNCH("rademacher");
  return LDMAE_OK;
}

extern "C" int ldmae_normal_f32(float* out, long n, unsigned long long seed, unsigned long long counter, void* stream) {
  LDMAE_REQUIRE(out && n > 0 && ((uintptr_t)out & 3) == 0, "normal: bad arguments (n = %ld)", n);
  LDMAE_REQUIRE(ode_items(n) <= 0x7fffffffL * ODE_BLOCK_ITEMS, "normal: n too large");
  hipLaunchKernelGGL(normal_kernel, dim3(ode_grid(n)), dim3(ODE_THREADS), 0, as_stream(stream), out, n, (unsigned)(seed & 0xffffffffu),
                     (unsigned)(seed >> 32), (unsigned)(counter & 0xffffffffu), (unsigned)(counter >> 32), al16(out) ? 1 : 0);
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
  LDMAE_REQUIRE(ode_items(n) <= 0x7fffffffL * ODE_BLOCK_ITEMS, "sde_combine: n too large");
  SdeIn a;
  const float* in[4] = {in0, in1, in2, in3};
  for (int j = 0; j < 4; ++j) {
    a.p[j] = j < m ? in[j] : nullptr;
    a.c[j] = j < m ? coef[j] : 0.f;
    LDMAE_REQUIRE(j >= m || (in[j] && al16(in[j])), "sde_combine: input %d is null or not 16-byte aligned", j);
  }
  LDMAE_REQUIRE(al16(out) && al16(mean_out) && al16(z), "sde_combine: out, mean_out and z must be 16-byte aligned");
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
  switch (m) {
    case 1: launch_sde_combine<1>(noise_mode, a, z, noise_coef, seed, counter, out, mean_out, n, t_next, t_out, nt, st); break;
    case 2: launch_sde_combine<2>(noise_mode, a, z, noise_coef, seed, counter, out, mean_out, n, t_next, t_out, nt, st); break;
    case 3: launch_sde_combine<3>(noise_mode, a, z, noise_coef, seed, counter, out, mean_out, n, t_next, t_out, nt, st); break;
    default: launch_sde_combine<4>(noise_mode, a, z, noise_coef, seed, counter, out, mean_out, n, t_next, t_out, nt, st); break;
  }
  LDMAE_CHECK_LAUNCH("sde_combine");
  return LDMAE_OK;
}

extern "C" long ldmae_rowdot_partials(int B, long m) { return (B > 0 && m > 0) ? (long)B * cdiv(m, ROW_CHUNK) : 0; }

extern "C" int ldmae_rowdot_f32(const float* a, const float* b, float* out, int B, long m, float* partial, void* stream) {
  LDMAE_REQUIRE(a && b && out && partial && B > 0 && m > 0, "rowdot: bad arguments (B = %d, m = %ld)", B, m);
  LDMAE_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "rowdot: a and b must be 4-byte aligned");
  const long chunks = cdiv(m, ROW_CHUNK);
  LDMAE_REQUIRE((long)B * chunks <= 0x7fffffffL, "rowdot: B * ceil(m / 4096) = %ld blocks is too many", (long)B * chunks);
  const int vec = (al16(a) && al16(b) && (B == 1 || (m & 3) == 0)) ? 1 : 0;      // every row start 16-byte aligned
  hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)(B * chunks)), dim3(ODE_THREADS), 0, as_stream(stream), a, b, partial, m, chunks, vec);
  hipLaunchKernelGGL(rowdot_fold_kernel, dim3(B), dim3(ODE_THREADS), 0, as_stream(stream), partial, chunks, out);
  LDMAE_CHECK_LAUNCH("rowdot");
  return LDMAE_OK;
}

extern "C" int ldmae_likelihood_finish_f32(const float* sumsq, const float* delta, float c, float* logp, int B, void* stream) {
  LDMAE_REQUIRE(sumsq && delta && logp && B > 0, "likelihood_finish: bad arguments");
  hipLaunchKernelGGL(likelihood_finish_kernel, dim3(cdiv(B, 256)), dim3(256), 0, as_stream(stream), sumsq, delta, c, logp, B);
  LDMAE_CHECK_LAUNCH("likelihood_finish");
  return LDMAE_OK;
}
