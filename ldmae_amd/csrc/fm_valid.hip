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
// The loss.  loss[b] = (sum_j (float(a[b, j]) - u[b, j])^2) / m is the two-stage row reduction of flat_common.h, the one ldmae_rowdot_f32
// uses (chunk map, partial layout and summation order are written there and in DESIGN.md section 27): per element d = a - u rounded, then one
// fma into the thread's chain; the folded sum is divided by m.  The order depends on (m, alignment) only: two runs give the same bits.
#include "flat_common.h"
#include "philox_normal.h"

// Every rounding below is written down: the compiler fuses no multiply with an add in this file (hipcc's default would), an fma is spelled
// fmaf.  Plain operators on purpose: __fmul_rn / __fadd_rn are inline functions of a header compiled BEFORE this pragma, so a product and a sum
// written with them may still be contracted into one fma after inlining.
#pragma clang fp contract(off)

namespace {

constexpr int FMV_THREADS = 256;

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

// the term and the result of the row reduction (row_reduce of flat_common.h): d = a - u rounded, one fma; the sum divided by m
struct MseTerm {
  __device__ float operator()(float a, float u, float s) const {
    const float d = a - u;
    return __builtin_fmaf(d, d, s);
  }
};
struct MeanFinish {
  float m;
  __device__ float operator()(float s) const { return s / m; }
};

}  // namespace

extern "C" int ldmae_fm_valid_plan_f32(const float* stored, const long long* idx, const float* t, const float* lat_mean, const float* lat_std,
                                       float multiplier, int sample, unsigned long long seed, float* xt, float* ut, int B, int C, int HW,
                                       void* stream) {
  LDMAE_REQUIRE(stored && idx && t && xt && ut && B > 0 && C > 0 && HW > 0, "fm_valid_plan: null pointer or empty input");
  LDMAE_REQUIRE(HW % 4 == 0, "fm_valid_plan: H*W=%d must be a multiple of 4", HW);
  LDMAE_REQUIRE((lat_mean == nullptr) == (lat_std == nullptr), "fm_valid_plan: give both latent mean and std, or neither");
  LDMAE_REQUIRE(sample == 0 || sample == 1, "fm_valid_plan: sample is 0 or 1, got %d", sample);
  LDMAE_REQUIRE(is_aligned(stored) && is_aligned(xt) && is_aligned(ut), "fm_valid_plan: stored, xt and ut must be 16-byte aligned");
  LDMAE_REQUIRE((((uintptr_t)idx & 7) | ((uintptr_t)t & 3)) == 0, "fm_valid_plan: idx must be 8-byte and t 4-byte aligned");
  const long n = (long)C * HW, n4 = n >> 2;
  LDMAE_REQUIRE(xt + (size_t)B * n <= ut || ut + (size_t)B * n <= xt, "fm_valid_plan: xt and ut overlap");
  const long bps = cdiv(n4, FMV_THREADS);
  const PhiloxWords key(seed, 0);
  LDMAE_REQUIRE((long)B * bps <= 0x7fffffffL, "fm_valid_plan: B * ceil(C*HW / 1024) = %ld blocks is too many", (long)B * bps);
  hipLaunchKernelGGL(fm_valid_plan_kernel, dim3((unsigned)(B * bps)), dim3(FMV_THREADS), 0, as_stream(stream), stored, idx, t, lat_mean, lat_std,
                     multiplier, sample, key.k0, key.k1, xt, ut, C, HW, n4, (unsigned)bps);
  LDMAE_CHECK_LAUNCH("fm_valid_plan");
  return LDMAE_OK;
}

extern "C" long ldmae_row_mse_partials(int B, long m) { return row_partials(B, m); }

extern "C" int ldmae_row_mse(int a_dtype, const void* a, const float* u, float* loss, int B, long m, float* partial, void* stream) {
  LDMAE_REQUIRE(a_dtype == LDMAE_F32 || a_dtype == LDMAE_BF16, "row_mse: dtype %d (f32 or bf16)", a_dtype);
  LDMAE_REQUIRE(a && u && loss && partial && B > 0 && m > 0, "row_mse: bad arguments (B = %d, m = %ld)", B, m);
  LDMAE_REQUIRE(row_fits_grid(B, m), "row_mse: B * ceil(m / 4096) = %ld blocks is too many", (long)B * row_chunks(m));
  const int esize = a_dtype == LDMAE_BF16 ? 2 : 4;
  LDMAE_REQUIRE(is_aligned(a, esize) && is_aligned(u, 4), "row_mse: a and u must be aligned to their element size");
  // every row start aligned for a 4-element load: 16 bytes of f32, 8 bytes of bf16
  const int vec = row_vec(is_aligned(a, 4 * esize), is_aligned(u), B, m);
  auto go = [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    row_reduce<MseTerm>((const T*)a, u, loss, B, m, partial, vec, MeanFinish{(float)m}, as_stream(stream));
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(a_dtype, go)), "row_mse: dtype %d (f32 or bf16)", a_dtype);
  LDMAE_CHECK_LAUNCH("row_mse");
  return LDMAE_OK;
}
