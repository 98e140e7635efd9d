// The fp16-MFMA main loop of the TF32-class implicit-GEMM convolutions (conv_vae.hip: the *_f16 entry points).  Operands are fp16 (rounded
// once by the caller's fetch), products are exact in f32 and accumulated in f32 on v_mfma_f32_16x16x32_f16.
// 128 (M) x 128 (N) output tile, 256 threads = 2 x 2 waves of 64 x 64 (4 x 4 MFMA blocks of 16 x 16), BK = 32, register-staged double-
// buffered LDS.  K order inside a BK step is the natural one: lane group q = lane >> 4 of the MFMA takes k = 8 q .. 8 q + 7, one
// ds_read_b128 per 16 x 32 fragment, so a step costs a wave 8 ds_read_b128 for 16 MFMAs (half a read per 16-cycle MFMA).  Row stride 48
// halves = 96 B: with rows lane & 15 and 16-B chunks lane >> 4, each 16-lane group of a ds_read_b128 covers the 64 banks once (80 B, the
// byte stride of conv_igemm_f32.h, puts two lanes of a group on the same banks).
// Summation order is fixed by the shape alone: K steps in order, inside a step the MFMA's own order; no split K, no atomics.
// The element type T and with it the MFMA are template parameters, deduced from the LDS arrays: f16 (the default everywhere above) or bf16
// (v_mfma_f32_16x16x32_bf16: the LPIPS data gradient of lpips_f16.hip, whose operands need f32's exponent range).
#pragma once
#include "conv_igemm_common.h"

constexpr int CH_BM = 128, CH_BN = 128, CH_BK = 32, CH_LD = 48, CH_NT = 256;
typedef ConvTile<CH_BM, CH_BN, 8> ChTile;

template <class T> struct ConvMfma16;
template <> struct ConvMfma16<f16> {
  static __device__ __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct ConvMfma16<bf16> {
  static __device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// Staging: thread tid owns k-columns [lc, lc + 8) of rows lr and lr + 64 of A and of B (lr = tid >> 2, lc = (tid & 3) * 8).
// fetch_a(p) -> the eight fp16 of A row lr + 64 p at the caller's cursor; fetch_b(p, k0) -> those of B row lr + 64 p at K-step k0;
// advance() moves the caller's (tap, channel) cursor by one BK step.  They are called in this order once per step, one step ahead of the
// MFMAs.  acc[i][j]: D row (lane >> 4) * 4 + r, column lane & 15 of the 16 x 16 block (i, j) of this wave's 64 x 64 tile
// (wm = wave >> 1, wn = wave & 1).
template <class T = f16, class MMA = ConvMfma16<T>, class FetchA, class FetchB, class Advance>
__device__ __forceinline__ void conv_igemm_f16_mainloop(T (&As)[2][CH_BM * CH_LD], T (&Bs)[2][CH_BN * CH_LD], int nk, FetchA fetch_a,
                                                        FetchB fetch_b, Advance advance, f32x4 (&acc)[4][4]) {
  typedef typename Pack<T>::v8 vec8;                     // the 16-B fragment of the element type
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = tid >> 2, lc = (tid & 3) * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  vec8 ra0 = fetch_a(0), ra1 = fetch_a(1), rb0 = fetch_b(0, 0), rb1 = fetch_b(1, 0);
  advance();
  *(vec8*)&As[0][lr * CH_LD + lc] = ra0;
  *(vec8*)&As[0][(lr + 64) * CH_LD + lc] = ra1;
  *(vec8*)&Bs[0][lr * CH_LD + lc] = rb0;
  *(vec8*)&Bs[0][(lr + 64) * CH_LD + lc] = rb1;
  __syncthreads();
  const int q8 = (lane >> 4) * 8, r16 = lane & 15;
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      ra0 = fetch_a(0);
      ra1 = fetch_a(1);
      rb0 = fetch_b(0, (kt + 1) * CH_BK);
      rb1 = fetch_b(1, (kt + 1) * CH_BK);
      advance();
    }
    vec8 af[4], bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *(const vec8*)&As[cur][(wm * 64 + i * 16 + r16) * CH_LD + q8];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = *(const vec8*)&Bs[cur][(wn * 64 + j * 16 + r16) * CH_LD + q8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = MMA::mma(af[i], bf[j], acc[i][j]);
    if (kt + 1 < nk) {
      *(vec8*)&As[cur ^ 1][lr * CH_LD + lc] = ra0;
      *(vec8*)&As[cur ^ 1][(lr + 64) * CH_LD + lc] = ra1;
      *(vec8*)&Bs[cur ^ 1][lr * CH_LD + lc] = rb0;
      *(vec8*)&Bs[cur ^ 1][(lr + 64) * CH_LD + lc] = rb1;
    }
    __syncthreads();
    cur ^= 1;
  }
}
