// Held-out validation of the flow-matching objective (ldmae_amd/validate.py): the model input and the regression target of a validation batch
// from NAMED draws, and the per-sample squared error.  All f32 arithmetic, plain vector code, no atomics, fixed summation order.
//
// The plan.  Validation sample i (a global index, whatever batch or rank it lands in) owns two draws of n = C HW normals each:
// z = normal(seed, 2 i) for the posterior sample and x0 = normal(seed, 2 i + 1) for the noise end of the path -- bit for bit what
// ldmae_normal_f32(out, n, seed, counter) writes (philox_normal.h).  One thread owns the four consecutive elements 4 v .. 4 v + 3 of a sample:
// one Philox block of each stream, one 16-byte load per stored half, two 16-byte stores.  Neither draw is stored: 8 B read (mean, logvar) and
// 8 B written (xt, ut) per element.  HW % 4 == 0, so the four elements share their channel.
//   x1 = ((mean + exp(0.5 clamp(logvar, -30, 20)) z) - lat_mean[c]) / lat_std[c] * multiplier      ldmae_latent_prologue's expression (vmae.hip)
//   xt = t x1 + (1 - t) x0        1 - t rounded, each product rounded, the sum rounded (transport/path.py ICPlan.plan in f32, no contraction)
//   ut = x1 - x0
//
// The loss.  loss[b] = (sum_j (float(a[b, j]) - u[b, j])^2) / m, two-stage like ldmae_rowdot_f32: block (b, c) owns the 4096 elements
// [4096 c, 4096 c + 4096) of row b; vec (every row start of a and u aligned for a 4-element load): thread t takes the 4-element groups t,
// t + 256, t + 512, t + 768 of the chunk, element order inside each; otherwise thread t takes the elements t, t + 256, ... (16 of them).  Per
// element d = a - u rounded, then one fma chain per thread; a wave joins its lanes in the xor butterfly 32 .. 1, the four waves are added as
// (w0 + w1) + (w2 + w3); partial[b * chunks + c].  Stage 2: one block per row lets thread t add partial[t], partial[t + 256], ... in that order,
// joins the 256 threads the same way and divides by m.  The order depends on (m, alignment) only: two runs give the same bits.
#include "common.h"
#include "philox_normal.h"

// Every rounding below is written down: the compiler fuses no multiply with an add in this file (hipcc's default would), an fma is spelled
// fmaf.  Plain operators on purpose: __fmul_rn / __fadd_rn are inline functions of a header compiled BEFORE this pragma, so a product and a sum
// written with them may still be contracted into one fma after inlining.
#pragma clang fp contract(off)

namespace {

constexpr int FMV_THREADS = 256;
constexpr long MSE_CHUNK = 4096;

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ldmae_latent_prologue's arithmetic on one element (vmae.hip latent_prologue_kernel): mean + std * noise is ONE fma there (hipcc contracts
// `v += exp(..) * e`), the subtraction, the true division and the multiplication are rounded one by one
__device__ __forceinline__ float latent_x1(float v, float l, float e, float mu, float sd, float mult, bool sample, bool norm) {
  if (sample) v = __builtin_fmaf(expf(0.5f * fminf(fmaxf(l, -30.f), 20.f)), e, v);
  if (norm) v = (v - mu) / sd;
  else v -= mu;
  return v * mult;
}

__global__ __launch_bounds__(FMV_THREADS) void fm_valid_plan_kernel(const float* __restrict__ stored, const long long* __restrict__ idx,
                                                                    const float* __restrict__ t, const float* __restrict__ lmean,
                                                                    const float* __restrict__ lstd, float mult, int sample, unsigned k0, unsigned k1,
                                                                    float* __restrict__ xt, float* __restrict__ ut, int C, int HW, long n4,
                                                                    unsigned bps) {
  const unsigned b = blockIdx.x / bps;
  const long v = (long)(blockIdx.x - b * bps) * FMV_THREADS + threadIdx.x;      // the item (= Philox block) within the sample
  if (v >= n4) return;
  const long e = v << 2;
  const int c = (int)(e / HW);
  const long i = e - (long)c * HW;
  const unsigned long long ctr = 2ull * (unsigned long long)idx[b];             // mod 2^64
  float z[4] = {0.f, 0.f, 0.f, 0.f}, x0[4];
  if (sample) philox_normal4(v, k0, k1, (unsigned)(ctr & 0xffffffffu), (unsigned)(ctr >> 32), z);
  philox_normal4(v, k0, k1, (unsigned)((ctr + 1) & 0xffffffffu), (unsigned)((ctr + 1) >> 32), x0);
  const float* m = stored + ((size_t)b * (sample ? 2 * C : C) + c) * HW + i;
  const float4 mv = *(const float4*)m;
  const float4 lv = sample ? *(const float4*)(m + (size_t)C * HW) : make_float4(0.f, 0.f, 0.f, 0.f);
  const bool norm = lstd != nullptr;
  const float mu = lmean ? lmean[c] : 0.f, sd = norm ? lstd[c] : 1.f;
  const float x1[4] = {latent_x1(mv.x, lv.x, z[0], mu, sd, mult, sample, norm), latent_x1(mv.y, lv.y, z[1], mu, sd, mult, sample, norm),
                       latent_x1(mv.z, lv.z, z[2], mu, sd, mult, sample, norm), latent_x1(mv.w, lv.w, z[3], mu, sd, mult, sample, norm)};
  const float tb = t[b], omt = 1.f - tb;
  float a[4], u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = tb * x1[j] + omt * x0[j];
    u[j] = x1[j] - x0[j];
  }
  const size_t o = (size_t)b * ((size_t)n4 << 2) + e;
  *(float4*)(xt + o) = make_float4(a[0], a[1], a[2], a[3]);
  *(float4*)(ut + o) = make_float4(u[0], u[1], u[2], u[3]);
}

__device__ __forceinline__ float block_sum(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float mse_term(float a, float u, float s) {
  const float d = a - u;
  return __builtin_fmaf(d, d, s);
}

__device__ __forceinline__ float4 load4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 load4(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

template <typename T>
__global__ __launch_bounds__(FMV_THREADS) void row_mse_kernel(const T* __restrict__ a, const float* __restrict__ u, float* __restrict__ partial, long m,
                                                              long chunks, int vec) {
  __shared__ float red[4];
  const long r = blockIdx.x / chunks, c = blockIdx.x - r * chunks;
  const T* ar = a + r * m;
  const float* ur = u + r * m;
  const long lo = c * MSE_CHUNK, hi = lo + MSE_CHUNK < m ? lo + MSE_CHUNK : m;
  float s = 0.f;
  if (vec) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long e = lo + 4 * ((long)threadIdx.x + (long)k * FMV_THREADS);
      if (e + 4 <= hi) {
        const float4 x = load4(ar + e), y = load4(ur + e);
        s = mse_term(x.x, y.x, s); s = mse_term(x.y, y.y, s); s = mse_term(x.z, y.z, s); s = mse_term(x.w, y.w, s);
      } else {
        for (long i = e; i < hi; ++i) s = mse_term(to_f<T>(ar[i]), ur[i], s);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const long i = lo + threadIdx.x + (long)k * FMV_THREADS;
      if (i < hi) s = mse_term(to_f<T>(ar[i]), ur[i], s);
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(FMV_THREADS) void row_mse_fold_kernel(const float* __restrict__ partial, long chunks, float m, float* __restrict__ out) {
  __shared__ float red[4];
  const float* p = partial + (long)blockIdx.x * chunks;
  float s = 0.f;
  for (long i = threadIdx.x; i < chunks; i += FMV_THREADS) s += p[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s / m;
}

}  // namespace

extern "C" int ldmae_fm_valid_plan_f32(const float* stored, const long long* idx, const float* t, const float* lat_mean, const float* lat_std,
                                       float multiplier, int sample, unsigned long long seed, float* xt, float* ut, int B, int C, int HW,
                                       void* stream) {
  LDMAE_REQUIRE(stored && idx && t && xt && ut && B > 0 && C > 0 && HW > 0, "fm_valid_plan: null pointer or empty input");
  LDMAE_REQUIRE(HW % 4 == 0, "fm_valid_plan: H*W=%d must be a multiple of 4", HW);
  LDMAE_REQUIRE((lat_mean == nullptr) == (lat_std == nullptr), "fm_valid_plan: give both latent mean and std, or neither");
  LDMAE_REQUIRE(sample == 0 || sample == 1, "fm_valid_plan: sample is 0 or 1, got %d", sample);
  LDMAE_REQUIRE(al16(stored) && al16(xt) && al16(ut), "fm_valid_plan: stored, xt and ut must be 16-byte aligned");
  LDMAE_REQUIRE((((uintptr_t)idx & 7) | ((uintptr_t)t & 3)) == 0, "fm_valid_plan: idx must be 8-byte and t 4-byte aligned");
  const long n = (long)C * HW, n4 = n >> 2;
  LDMAE_REQUIRE(xt + (size_t)B * n <= ut || ut + (size_t)B * n <= xt, "fm_valid_plan: xt and ut overlap");
  const long bps = cdiv(n4, FMV_THREADS);
  LDMAE_REQUIRE((long)B * bps <= 0x7fffffffL, "fm_valid_plan: B * ceil(C*HW / 1024) = %ld blocks is too many", (long)B * bps);
  hipLaunchKernelGGL(fm_valid_plan_kernel, dim3((unsigned)(B * bps)), dim3(FMV_THREADS), 0, as_stream(stream), stored, idx, t, lat_mean, lat_std,
                     multiplier, sample, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), xt, ut, C, HW, n4, (unsigned)bps);
  LDMAE_CHECK_LAUNCH("fm_valid_plan");
  return LDMAE_OK;
}

extern "C" long ldmae_row_mse_partials(int B, long m) { return (B > 0 && m > 0) ? (long)B * cdiv(m, MSE_CHUNK) : 0; }

extern "C" int ldmae_row_mse(int a_dtype, const void* a, const float* u, float* loss, int B, long m, float* partial, void* stream) {
  LDMAE_REQUIRE(a_dtype == LDMAE_F32 || a_dtype == LDMAE_BF16, "row_mse: dtype %d (f32 or bf16)", a_dtype);
  LDMAE_REQUIRE(a && u && loss && partial && B > 0 && m > 0, "row_mse: bad arguments (B = %d, m = %ld)", B, m);
  const long chunks = cdiv(m, MSE_CHUNK);
  LDMAE_REQUIRE((long)B * chunks <= 0x7fffffffL, "row_mse: B * ceil(m / 4096) = %ld blocks is too many", (long)B * chunks);
  const int esize = a_dtype == LDMAE_BF16 ? 2 : 4;
  LDMAE_REQUIRE(((uintptr_t)a & (esize - 1)) == 0 && ((uintptr_t)u & 3) == 0, "row_mse: a and u must be aligned to their element size");
  // every row start aligned for a 4-element load: 16 bytes of f32, 8 bytes of bf16
  const int vec = (((uintptr_t)a & (4 * esize - 1)) == 0 && al16(u) && (B == 1 || (m & 3) == 0)) ? 1 : 0;
  hipStream_t st = as_stream(stream);
  auto go = [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    hipLaunchKernelGGL(row_mse_kernel<T>, dim3((unsigned)(B * chunks)), dim3(FMV_THREADS), 0, st, (const T*)a, u, partial, m, chunks, vec);
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(a_dtype, go)), "row_mse: dtype %d (f32 or bf16)", a_dtype);
  hipLaunchKernelGGL(row_mse_fold_kernel, dim3(B), dim3(FMV_THREADS), 0, st, partial, chunks, (float)m, loss);
  LDMAE_CHECK_LAUNCH("row_mse");
  return LDMAE_OK;
}
