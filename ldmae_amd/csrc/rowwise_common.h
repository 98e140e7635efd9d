// Shared by elementwise.hip, qk_rope.hip, pointwise.hip and mx8.hip: four-channel loads / stores, float4 arithmetic, launch sizes, group_reduce.
#pragma once
#include "common.h"

// ------------------------------------------------------------------ small vector helpers
template <typename T> __device__ __forceinline__ float4 load4(const T* p);
template <> __device__ __forceinline__ float4 load4<float>(const float* p) { const f32x4 v = __builtin_nontemporal_load((const f32x4*)p); return make_float4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ float4 load4<bf16>(const bf16* p) {
  bf16x4 v = __builtin_nontemporal_load((const bf16x4*)p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
template <> __device__ __forceinline__ float4 load4<f16>(const f16* p) {
  const f16x4 a = *(const f16x4*)p;
  return make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
}
template <typename T> __device__ __forceinline__ void store4(T* p, float4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, float4 v) { f32x4 o = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(o, (f32x4*)p); }
template <> __device__ __forceinline__ void store4<bf16>(bf16* p, float4 v) {
  bf16x4 o; o[0] = (bf16)v.x; o[1] = (bf16)v.y; o[2] = (bf16)v.z; o[3] = (bf16)v.w;
  __builtin_nontemporal_store(o, (bf16x4*)p);
}
template <> __device__ __forceinline__ void store4<f16>(f16* p, float4 v) {
  f16x4 o; o[0] = from_f<f16>(v.x); o[1] = from_f<f16>(v.y); o[2] = from_f<f16>(v.z); o[3] = from_f<f16>(v.w);
  *(f16x4*)p = o;
}
__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float hsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// a product that is never contracted into a following add (HIP's __fmul_rn is a plain `*`): its consumers sum the value AS STORED
__device__ __forceinline__ float4 mul_rn(float4 a, float4 b) {
#pragma clang fp contract(off)
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// the fixed-order sum of partial rows (P2 / out2 / beta2: a second one of the same shape in the same launch); defined once, with its kernel, in elementwise.hip
void group_reduce(const float* P, int p_ld, int nout, int cols, int group, float* out, int out_ld, float beta, hipStream_t st,
                  const float* P2 = nullptr, float* out2 = nullptr, float beta2 = 0.f);

// rows per workgroup for the per-sample reductions: largest of 64/32/16/8/4 dividing rows_per_batch
static inline int pick_rows_per_wg(int rows_per_batch) {
  const int cap = ldmae_tune_get(10) > 0 ? ldmae_tune_get(10) : 64;      // tune key 10: A/B knob
  for (int r = cap; r >= 1; r >>= 1) if (rows_per_batch % r == 0) return r;      // (odd token counts -- a 5 x 5 grid -- end at 1 row per workgroup: correct, slow)
  return 0;
}
static inline unsigned ew_grid(long n) { long g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }
