// The exact-f32 MFMA main loop of the implicit-GEMM convolutions (inception.hip: forward; lpips_bwd.hip: data gradient).
// 128 (M) x 64 (N) output tile, 256 threads = 2 x 2 waves of 64 x 32 (4 x 2 MFMA blocks of 16 x 16), BK = 16, register-staged double-
// buffered LDS.  K order inside a BK step is permuted the same way for both operands: MFMA kk of lane group q = lane >> 4 takes k = 4 q + kk,
// so each lane fetches its four A (B) values of a step with ONE ds_read_b128 instead of four ds_read_b32.  The sum is over the same products,
// in a different order (f32 rounding only).  Row stride 20 floats: the eight 16-B reads of a ds_read_b128 phase hit disjoint banks.
#pragma once
#include "conv_igemm_common.h"

constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 16, CV_LD = 20, CV_NT = 256;
typedef ConvTile<CV_BM, CV_BN, 4> CvTile;

// Staging: thread tid owns k-columns [lc, lc + 4) of A rows lr and lr + 64 and of B row lr (lr = tid >> 2, lc = (tid & 3) * 4).
// fetch_a(p, k0) -> the float4 of A row lr + 64 p at K-step k0; fetch_b(k0) -> the float4 of B row lr; advance() moves the caller's (tap,
// channel) cursor by one BK step.  They are called in this order once per step, one step ahead of the MFMAs.
// acc[i][j]: D row (lane >> 4) * 4 + r, column lane & 15 of the 16 x 16 block (i, j) of this wave's 64 x 32 tile (wm = wave >> 1, wn = wave & 1).
template <class FetchA, class FetchB, class Advance>
__device__ __forceinline__ void conv_igemm_f32_mainloop(float (&As)[2][CV_BM * CV_LD], float (&Bs)[2][CV_BN * CV_LD], int nk, FetchA fetch_a,
                                                        FetchB fetch_b, Advance advance, f32x4 (&acc)[4][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = tid >> 2, lc = (tid & 3) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ra0 = fetch_a(0, 0), ra1 = fetch_a(1, 0), rb = fetch_b(0);
  advance();
  *(float4*)&As[0][lr * CV_LD + lc] = ra0;
  *(float4*)&As[0][(lr + 64) * CV_LD + lc] = ra1;
  *(float4*)&Bs[0][lr * CV_LD + lc] = rb;
  __syncthreads();
  const int q4 = (lane >> 4) * 4, r16 = lane & 15;
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      ra0 = fetch_a(0, (kt + 1) * CV_BK);
      ra1 = fetch_a(1, (kt + 1) * CV_BK);
      rb = fetch_b((kt + 1) * CV_BK);
      advance();
    }
    float4 af[4], bf[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *(const float4*)&As[cur][(wm * 64 + i * 16 + r16) * CV_LD + q4];
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[j] = *(const float4*)&Bs[cur][(wn * 32 + j * 16 + r16) * CV_LD + q4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
      }
    if (kt + 1 < nk) {
      *(float4*)&As[cur ^ 1][lr * CV_LD + lc] = ra0;
      *(float4*)&As[cur ^ 1][(lr + 64) * CV_LD + lc] = ra1;
      *(float4*)&Bs[cur ^ 1][lr * CV_LD + lc] = rb;
    }
    __syncthreads();
    cur ^= 1;
  }
}
