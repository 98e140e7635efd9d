// The tile skeleton around the two implicit-GEMM main loops (conv_igemm_f32.h, conv_igemm_f16.h): everything a convolution kernel does
// that is not its operand gather or its store.  M = output pixels, N = output channels, K = taps x gathered channels in (ky, kx, c) order.
// A kernel builds a ConvTile, decodes its two staged rows with conv_row, walks K with TAP_WRAP, fetches weights with conv_weight_row /
// fetch_weight_row, calls the main loop and hands CONV_EPILOGUE a store; its entry point launches through conv_launch.
// The tail rule has two halves and both live here: conv_row clamps the row it decodes and CONV_EPILOGUE guards the store (filters past N:
// conv_weight_row and the same guard).
// Every piece was checked to leave each kernel's code object as it was (tools/codeobj_diff.py: equal).  That is why the two loops are
// macros: the compiler simplifies a function on its own before it inlines it, and a loop simplified ahead of the kernel around it comes
// out as other code than the same loop written in the kernel.
#pragma once
#include "common.h"

// Block -> output tile, and this thread's staging coordinates: thread tid owns the FW k-columns from lc of rows lr and lr + 64 (FW: elements
// of a 16-byte fragment, 4 f32 or 8 fp16 / bf16).
template <int BM, int BN, int FW>
struct ConvTile {
  int m0, n0, lr, lc;
  __device__ __forceinline__ explicit ConvTile(int N) {
    const int tid = threadIdx.x, tiles_n = (N + BN - 1) / BN;
    m0 = (int)(blockIdx.x / tiles_n) * BM; n0 = (int)(blockIdx.x % tiles_n) * BN;
    lr = tid >> 2; lc = (tid & 3) * FW;
  }
};

// Staged row p (0 or 1) of a tile: its image and the input coordinates of tap (0, 0).
struct ConvRow { int b, iy0, ix0; };
template <class Tile>
__device__ __forceinline__ ConvRow conv_row(const Tile& t, int p, int M, int Ho, int Wo, int sh, int sw, int ph, int pw) {
  const int m = min(t.m0 + t.lr + p * 64, M - 1);          // rows past M fetch a real pixel; their results are never stored
  const int ox = m % Wo, r = m / Wo, oy = r % Ho;
  return {r / Ho, oy * sh - ph, ox * sw - pw};
}

// The (tap, channel) cursor of a thread's fragment: channel ci of tap (ky, kx), advanced by BK per step without divisions.  C is a multiple
// of the fragment width, so a fragment never straddles a tap; a BK step may walk over several taps (C < BK), hence the loop.  ky reaches the
// kernel height past K.  The f32 and the KL-VAE kernels keep the three as locals (ci = lc, kx = ky = 0, TAP_WRAP; per step ci += BK,
// TAP_WRAP), the 16-bit LPIPS kernels as a TapCursor: the two spellings compile differently (members of one object are promoted to
// registers earlier), and each kernel keeps the one it was measured with.
#define TAP_WRAP(ci, kx, ky, C, kw) \
  while ((ci) >= (C)) { (ci) -= (C); if (++(kx) == (kw)) { (kx) = 0; ++(ky); } }
template <int BK>
struct TapCursor {
  int ci, kx, ky;
  __device__ __forceinline__ void init(int lc, int C, int kw) { ci = lc; kx = 0; ky = 0; wrap(C, kw); }
  __device__ __forceinline__ void wrap(int C, int kw) { TAP_WRAP(ci, kx, ky, C, kw) }
  __device__ __forceinline__ void step(int C, int kw) { ci += BK; wrap(C, kw); }
};

// Filter row n of w [N, K]; rows past N fetch the last filter, never stored.  One 16-byte fragment of it at k (K a multiple of the
// fragment width), zeros past K.
template <class T>
__device__ __forceinline__ const T* conv_weight_row(const T* w, int n, int N, int K) { return w + (size_t)min(n, N - 1) * K; }
template <class V, class T>
__device__ __forceinline__ V fetch_weight_row(const T* wrow, int k, int K) {
  if (k < K) return *(const V*)(wrow + k);
  return V{};
}

// The walk over a wave's accumulators acc[4][NJ].  256 threads = 2 x 2 waves; wave (wm, wn) owns rows [64 wm, 64 wm + 64) and columns
// [16 NJ wn, 16 NJ wn + 16 NJ) of the tile, and acc[i][j][r] is D row (lane >> 4) * 4 + r, column lane & 15 of its 16 x 16 block (i, j).
// For every column n < N: c = col(n) once, then store(m, n, acc[i][j][r], c) for its rows m < M.
// Written as a function, the walk is unrolled before it meets the kernel's accumulators, and every store pays one more 64-bit add.
#define CONV_EPILOGUE(acc, NJ, t, M, N, col, store)                               \
  do {                                                                            \
    const int lane_ = threadIdx.x & 63, wave_ = threadIdx.x >> 6, wm_ = wave_ >> 1, wn_ = wave_ & 1; \
    const int q4_ = (lane_ >> 4) * 4, r16_ = lane_ & 15;                          \
    _Pragma("unroll") for (int j_ = 0; j_ < (NJ); ++j_) {                         \
      const int n_ = (t).n0 + wn_ * ((NJ) * 16) + j_ * 16 + r16_;                 \
      if (n_ >= (N)) continue;                                                    \
      const auto c_ = col(n_);                                                    \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                            \
        _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                        \
          const int m_ = (t).m0 + wm_ * 64 + i_ * 16 + q4_ + r_;                  \
          if (m_ < (M)) store(m_, n_, (acc)[i_][j_][r_], c_);                     \
        }                                                                         \
    }                                                                             \
  } while (0)
// col of the kernels that add a bias: loaded once per column, NULL = none; and of those that add nothing
__device__ __forceinline__ auto conv_bias(const float* bias) {
  return [bias](int n) { return bias ? bias[n] : 0.f; };
}
__device__ __forceinline__ auto conv_no_col() {
  return [](int) { return 0; };
}

// Grid from (M, N) and the tile, the profiler bracket with 2 M N K flops, the launch and its check.
template <int BM, int BN, int NT, class... P, class... A>
static int conv_launch(const char* name, void (*kernel)(P...), long M, long N, long K, void* stream, A... args) {
  const unsigned grid = cdiv(M, BM) * cdiv(N, BN);
  const long pidx = ldmae_prof_is_on() ? ldmae_prof_begin(as_stream(stream), 2.0 * M * N * K) : -1;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, as_stream(stream), args...);
  if (pidx >= 0) ldmae_prof_end(pidx, as_stream(stream));
  LDMAE_CHECK_LAUNCH(name);
  return 0;
}
