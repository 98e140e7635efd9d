// ADM evaluator (the reference's tools/evaluator.py: Inception Score, FID, sFID, precision and recall), f32 on gfx950.
//   - TF-compatible pre-processing of the Inception graph (ExpandDims -> ResizeBilinear(299, 299) -> Sub 128 -> Mul 1/128);
//   - the sFID spatial tap: channels [0, 7) of Mixed_6d's output (TF mixed_6/conv), flattened in TF's NHWC order;
//   - f64 row norms |u|^2 rounded to f32 once;
//   - one NT pairwise GEMM core U[M, D] . V[N, D]^T on the exact-f32 MFMA with three epilogues: plain logits, per-row k smallest squared
//     distances (k-NN radii) and the precision / recall membership flags; two more for KID (polynomial-kernel sums in f64 over index
//     subsets) and for density / coverage (per-row ball counts);
//   - the softmax + Inception Score sums in f64 with fixed-order partials.
#include "common.h"

// ------------------------------------------------------------------------------------------------ pre-processing (TF1 ResizeBilinear)
// Specification (TF1's legacy rule: align_corners = False, half_pixel_centers = False), per output pixel (oy, ox) and channel:
//   scale = in / out                       (f32 division, per axis)
//   src   = dst * scale                    (f32)
//   lo    = floor(src),  hi = min(lo + 1, in - 1),  lerp = src - lo
//   top = tl + (tr - tl) * xl,  bot = bl + (br - bl) * xl,  v = top + (bot - top) * yl     (raw 0..255 floats, f32, no contraction)
//   out = (v - 128) * 0.0078125
// lo is clamped to in - 1 as well (never reached for out >= 1: src < in), so no read leaves the image.
__global__ __launch_bounds__(256) void adm_preprocess_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int B, int H, int W, int Ho,
                                                             int Wo) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Wo) return;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), b = (int)(i / ((long)Wo * Ho));
  const float shf = (float)H / (float)Ho, swf = (float)W / (float)Wo;
  const float sy = (float)oy * shf, sx = (float)ox * swf;
  const float fy = floorf(sy), fx = floorf(sx);
  const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float yl = sy - fy, xl = sx - fx;
  const uint8_t* base = img + (size_t)b * H * W * 3;
  const uint8_t *p00 = base + ((size_t)y0 * W + x0) * 3, *p01 = base + ((size_t)y0 * W + x1) * 3;
  const uint8_t *p10 = base + ((size_t)y1 * W + x0) * 3, *p11 = base + ((size_t)y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = (float)p00[c], tr = (float)p01[c], bl = (float)p10[c], br = (float)p11[c];
    const float top = tl + (tr - tl) * xl;
    const float bot = bl + (br - bl) * xl;
    const float v = top + (bot - top) * yl;
    out[i * 3 + c] = (v - 128.f) * 0.0078125f;
  }
}

extern "C" int ldmae_adm_preprocess(const unsigned char* img, float* out, int B, int H, int W, int Ho, int Wo, void* stream) {
  LDMAE_REQUIRE(img && out && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "adm_preprocess: bad arguments");
  hipLaunchKernelGGL(adm_preprocess_kernel, dim3(cdiv((long)B * Ho * Wo, 256)), dim3(256), 0, as_stream(stream), img, out, B, H, W, Ho, Wo);
  LDMAE_CHECK_LAUNCH("adm_preprocess");
  return 0;
}

// ------------------------------------------------------------------------------------------------ spatial tap
// out[b, p * C + c] = x[b, p, xoff + c]: a channel slice of an NHWC tensor made contiguous, i.e. flattened in (h, w, c) order
__global__ __launch_bounds__(256) void adm_spatial_tap_kernel(const float* __restrict__ x, int ldx, int xoff, float* __restrict__ out, int B, int HW,
                                                              int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * HW * C) return;
  const long pix = i / C;
  out[i] = x[pix * ldx + xoff + (int)(i % C)];
}

extern "C" int ldmae_adm_spatial_tap(const float* x, int ldx, int xoff, float* out, int B, int HW, int C, void* stream) {
  LDMAE_REQUIRE(x && out && B > 0 && HW > 0 && C > 0 && xoff >= 0 && xoff + C <= ldx, "adm_spatial_tap: bad arguments");
  hipLaunchKernelGGL(adm_spatial_tap_kernel, dim3(cdiv((long)B * HW * C, 256)), dim3(256), 0, as_stream(stream), x, ldx, xoff, out, B, HW, C);
  LDMAE_CHECK_LAUNCH("adm_spatial_tap");
  return 0;
}

// ------------------------------------------------------------------------------------------------ row norms
// one wave per row: lane partial sums over d = lane, lane + 64, ... in f64, then a fixed butterfly; rounded to f32 once
__global__ __launch_bounds__(256) void row_sqnorms_kernel(const float* __restrict__ x, int M, int D, float* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* p = x + (size_t)row * D;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)p[d];
    s = fma(v, v, s);
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = (float)s;
}

extern "C" int ldmae_row_sqnorms_f32(const float* x, int M, int D, float* out, void* stream) {
  LDMAE_REQUIRE(x && out && M > 0 && D > 0, "row_sqnorms_f32: bad arguments");
  hipLaunchKernelGGL(row_sqnorms_kernel, dim3(cdiv(M, 4)), dim3(256), 0, as_stream(stream), x, M, D, out);
  LDMAE_CHECK_LAUNCH("row_sqnorms_f32");
  return 0;
}

// ------------------------------------------------------------------------------------------------ NT pairwise GEMM core
// The convolution kernel's tile (inception.hip): 128 (M) x 64 (N) outputs, 256 threads = 2 x 2 waves of 64 x 32 (4 x 2 MFMA blocks of
// 16 x 16), BK = 16, register-staged double-buffered LDS, one ds_read_b128 per operand and step (K permuted the same way for both operands).
// A workgroup owns one row tile and walks the column tiles [s * tps, (s + 1) * tps) of its column split s; split boundaries are whole tiles,
// so an element (i, j) is computed at the same place of the same tile shape, over the same K order, whatever the split count: every
// distance is bitwise the same value for every split, and a selection from them does not depend on the split either.
//   PW_LOGITS: out[i, j] = u_i . v_j (plain f32 store).
//   PW_KNN:    d = max((|u|^2 - 2 u.v) + |v|^2, 0); each (row, split, half of the tile's columns) keeps its KNN_KP smallest d, ascending,
//              in registers and writes them as one partial list.
//   PW_PR:     the same d; u_in[i, k] = 1 if some column j has d <= rv[j, k]; v_in[j, k] = 1 if some row i has d <= ru[i, k]: plain stores
//              of 1 into flags the caller zeroed (an OR: idempotent, no ordering needed).
//   PW_COUNT:  the same d; each (row, split, half of the tile's columns) counts its columns with d < ru[i] (strictly) and writes the count as
//              one integer partial; count_merge_kernel adds a row's partials (integers: no order to fix).
//   PW_KID:    rows are read THROUGH an index table (row i of the operand is x[idx[i]], never gathered); blockIdx.y = 3 s + which picks the
//              subset s and the pair which = 0: (a, a), 1: (b, b), 2: (a, b).  Per element p = fmaf(gamma, u.v, coef0), p3 = (p * p) * p with
//              one rounding per step; p3 is added in f64 over the valid elements (i < m, j < m, and i != j for which < 2: both sides are the
//              same subset, so the position diagonal is the trace).  A thread adds its 32 elements in (j, i, r) order, the 64 lanes fold in
//              a butterfly, the four wave sums as (w0 + w1) + (w2 + w3): one f64 partial per (s, which, row tile, column tile) -- per TILE, not
//              per split, so kid_fold_kernel's sum over the tiles in ascending (row tile, column tile) order is the same bits for every nsplit.
constexpr int PW_BM = 128, PW_BN = 64, PW_BK = 16, PW_LD = 20, PW_NT = 256, PW_DLD = PW_BN + 1;
constexpr int KNN_KP = 8;           // list length: radii for neighbourhood sizes 0..7 (sorted index k, self-distance included)
constexpr int PR_MAXK = 8;          // at most 8 neighbourhood sizes
enum { PW_LOGITS = 0, PW_KNN = 1, PW_PR = 2, PW_KID = 3, PW_COUNT = 4 };

struct PairArgs {
  const float *u, *v, *nu, *nv, *ru, *rv;
  int M, N, D, nsplit, tps, nk;
  float* out;                        // PW_LOGITS: [M, N]; PW_KNN: partials [M, nsplit, 2, KNN_KP]
  int *u_in, *v_in;                  // PW_PR: [M, nk], [N, nk]; PW_COUNT: u_in = partials [M, nsplit, 2]
};
// PW_KID alone takes more (the other modes keep PairArgs as their kernel argument): u = a, v = b, M = N = m
struct KidArgs : PairArgs {
  const int *idx_u, *idx_v;          // [S, m]
  double* part;                      // [S, 3, row tiles, column tiles]
  float gamma, coef0;
};
template <int MODE> struct PairArgsOf { using type = PairArgs; };
template <> struct PairArgsOf<PW_KID> { using type = KidArgs; };

template <int MODE, bool VEC>
__global__ __launch_bounds__(PW_NT) void pairwise_kernel(typename PairArgsOf<MODE>::type a) {
  constexpr int STAGE = 2 * PW_BM * PW_LD + 2 * PW_BN * PW_LD, DIST = PW_BM * PW_DLD;
  __shared__ __attribute__((aligned(16))) float smem[STAGE > DIST ? STAGE : DIST];
  __shared__ float Ru[MODE == PW_PR ? PW_BM * PR_MAXK : 1], Rv[MODE == PW_PR ? PW_BN * PR_MAXK : 1];
  float* As0 = smem;                                        // As[buf] = smem + buf * BM * LD
  float* Bs0 = smem + 2 * PW_BM * PW_LD;                    // Bs[buf] = Bs0 + buf * BN * LD
  float* Ds = smem;                                         // [BM][DLD] distances, after the K loop
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int rt = (int)(blockIdx.x / a.nsplit), split = (int)(blockIdx.x % a.nsplit);
  const int m0 = rt * PW_BM;
  const float *ub = a.u, *vb = a.v;
  const int *iu = nullptr, *iv = nullptr;
  int which = 0;
  if constexpr (MODE == PW_KID) {
    which = (int)(blockIdx.y % 3);
    const size_t sub = (size_t)(blockIdx.y / 3) * a.M;
    iu = (which == 1 ? a.idx_v : a.idx_u) + sub;
    iv = (which == 0 ? a.idx_u : a.idx_v) + sub;
    ub = which == 1 ? a.v : a.u;
    vb = which == 0 ? a.u : a.v;
  }
  auto urow_of = [&](int pos) -> const float* {                // pos < M (clamped by the caller)
    if constexpr (MODE == PW_KID) return ub + (size_t)iu[pos] * a.D;
    return ub + (size_t)pos * a.D;
  };
  auto vrow_of = [&](int pos) -> const float* {
    if constexpr (MODE == PW_KID) return vb + (size_t)iv[pos] * a.D;
    return vb + (size_t)pos * a.D;
  };
  const int col_tiles = (a.N + PW_BN - 1) / PW_BN;
  const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, col_tiles);
  const int lr = tid >> 2, lc = (tid & 3) * 4;
  const float* urow[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) urow[p] = urow_of(min(m0 + lr + p * 64, a.M - 1));              // rows past M: real data, never stored
  const int q4 = (lane >> 4) * 4, r16 = lane & 15;

  // epilogue state: KNN lists of row er = tid >> 1, columns [eh * 32, eh * 32 + 32) of each tile; PR row bits of the same thread
  const int er = tid >> 1, eh = tid & 1;
  float best[KNN_KP];
#pragma unroll
  for (int q = 0; q < KNN_KP; ++q) best[q] = INFINITY;
  unsigned rowbits = 0;
  int count = 0;                                              // PW_COUNT: columns inside row er's ball, this thread's half of each tile
  float rrow = -1.f;                                          // d >= 0: a padded row counts nothing
  if constexpr (MODE == PW_COUNT) {
    if (m0 + er < a.M) rrow = a.ru[m0 + er];
  }
  if (MODE == PW_PR) {
    for (int e = tid; e < PW_BM * a.nk; e += PW_NT) {
      const int m = m0 + e / a.nk;
      Ru[e] = m < a.M ? a.ru[(size_t)m * a.nk + e % a.nk] : -1.f;      // d >= 0: a padded row is in nobody's ball
    }
  }

  auto fetch = [&](const float* row, int k) -> float4 {
    if constexpr (VEC) {
      if (k < a.D) return *(const float4*)(row + k);                 // D % 4 == 0: the whole float4 is in the row
      return make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = k + j < a.D ? row[k + j] : 0.f;
    return make_float4(t[0], t[1], t[2], t[3]);
  };

  const int nk_steps = (a.D + PW_BK - 1) / PW_BK;
  for (int ct = ct0; ct < ct1; ++ct) {
    const int n0 = ct * PW_BN;
    const float* vrow = vrow_of(min(n0 + lr, a.N - 1));
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 ra0 = fetch(urow[0], lc), ra1 = fetch(urow[1], lc), rb = fetch(vrow, lc);
    *(float4*)&As0[lr * PW_LD + lc] = ra0;
    *(float4*)&As0[(lr + 64) * PW_LD + lc] = ra1;
    *(float4*)&Bs0[lr * PW_LD + lc] = rb;
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk_steps; ++kt) {
      if (kt + 1 < nk_steps) {
        const int k = (kt + 1) * PW_BK + lc;
        ra0 = fetch(urow[0], k);
        ra1 = fetch(urow[1], k);
        rb = fetch(vrow, k);
      }
      const float* As = As0 + cur * PW_BM * PW_LD;
      const float* Bs = Bs0 + cur * PW_BN * PW_LD;
      float4 af[4], bf[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *(const float4*)&As[(wm * 64 + i * 16 + r16) * PW_LD + q4];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = *(const float4*)&Bs[(wn * 32 + j * 16 + r16) * PW_LD + q4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
      if (kt + 1 < nk_steps) {
        float* An = As0 + (cur ^ 1) * PW_BM * PW_LD;
        float* Bn = Bs0 + (cur ^ 1) * PW_BN * PW_LD;
        *(float4*)&An[lr * PW_LD + lc] = ra0;
        *(float4*)&An[(lr + 64) * PW_LD + lc] = ra1;
        *(float4*)&Bn[lr * PW_LD + lc] = rb;
      }
      __syncthreads();
      cur ^= 1;
    }
    // accumulator (row (lane >> 4) * 4 + r, column lane & 15 of each 16 x 16 block)
    if constexpr (MODE == PW_LOGITS) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 32 + j * 16 + r16;
        if (n >= a.N) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 64 + i * 16 + q4 + r;
            if (m < a.M) a.out[(size_t)m * a.N + n] = acc[i][j][r];
          }
      }
      continue;
    } else if constexpr (MODE == PW_KID) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 32 + j * 16 + r16;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 64 + i * 16 + q4 + r;
            if (m < a.M && n < a.N && (which == 2 || m != n)) {
              const float p = fmaf(a.gamma, acc[i][j][r], a.coef0);
              t += (double)__fmul_rn(__fmul_rn(p, p), p);
            }
          }
      }
      t = block_sum(t, (double*)smem);      // the staging buffers are free: the K loop ended on a barrier; free again for the next tile on return
      const size_t row_tiles = gridDim.x / a.nsplit;
      if (tid == 0) a.part[((size_t)blockIdx.y * row_tiles + rt) * col_tiles + ct] = t;
    } else {
      // distances of the tile into LDS (the staging buffers are free: the K loop ended on a barrier); padding is +inf
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cl = wn * 32 + j * 16 + r16, n = n0 + cl;
        const float nv = n < a.N ? a.nv[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rl = wm * 64 + i * 16 + q4 + r, m = m0 + rl;
            float d = INFINITY;
            if (m < a.M && n < a.N) {
              const float nu = a.nu[m];
              d = fmaxf(__fadd_rn(__fsub_rn(nu, 2.f * acc[i][j][r]), nv), 0.f);
            }
            Ds[rl * PW_DLD + cl] = d;
          }
      }
      if (MODE == PW_PR) {
        for (int e = tid; e < PW_BN * a.nk; e += PW_NT) {
          const int n = n0 + e / a.nk;
          Rv[e] = n < a.N ? a.rv[(size_t)n * a.nk + e % a.nk] : -1.f;
        }
      }
      __syncthreads();
      if constexpr (MODE == PW_KNN) {
        const float* drow = Ds + er * PW_DLD + eh * 32;
        for (int c = 0; c < 32; ++c) {
          const float v = drow[c];
          if (v < best[KNN_KP - 1]) {                                      // insert into the ascending list
#pragma unroll
            for (int q = KNN_KP - 1; q > 0; --q) best[q] = v < best[q - 1] ? best[q - 1] : (v < best[q] ? v : best[q]);
            best[0] = fminf(best[0], v);
          }
        }
      } else if constexpr (MODE == PW_COUNT) {
        const float* drow = Ds + er * PW_DLD + eh * 32;
        for (int c = 0; c < 32; ++c) count += drow[c] < rrow ? 1 : 0;      // padding is +inf: never inside
      } else {
        // rows: u_in[er, k] |= any over this thread's 32 columns of d <= rv[n, k]
        const float* drow = Ds + er * PW_DLD + eh * 32;
        for (int c = 0; c < 32; ++c) {
          const float d = drow[c];
          for (int k = 0; k < a.nk; ++k)
            if (d <= Rv[(eh * 32 + c) * a.nk + k]) rowbits |= 1u << k;
        }
        // columns: v_in[n, k] |= any over rows [wave * 32, wave * 32 + 32) of d <= ru[m, k]
        const int cl = lane, n = n0 + cl;
        unsigned colbits = 0;
        for (int rr = 0; rr < 32; ++rr) {
          const int rl = wave * 32 + rr;
          const float d = Ds[rl * PW_DLD + cl];
          for (int k = 0; k < a.nk; ++k)
            if (d <= Ru[rl * a.nk + k]) colbits |= 1u << k;
        }
        if (n < a.N && colbits)
          for (int k = 0; k < a.nk; ++k)
            if (colbits >> k & 1) a.v_in[(size_t)n * a.nk + k] = 1;
      }
      __syncthreads();                                                     // Ds / Rv are read before the next tile's staging
    }
  }
  const int m = m0 + er;
  if (MODE == PW_KNN && m < a.M) {
    float* dst = a.out + (((size_t)m * a.nsplit + split) * 2 + eh) * KNN_KP;
#pragma unroll
    for (int q = 0; q < KNN_KP; ++q) dst[q] = best[q];
  }
  if (MODE == PW_COUNT && m < a.M) a.u_in[((size_t)m * a.nsplit + split) * 2 + eh] = count;
  if (MODE == PW_PR && m < a.M && rowbits)
    for (int k = 0; k < a.nk; ++k)
      if (rowbits >> k & 1) a.u_in[(size_t)m * a.nk + k] = 1;
}

template <int MODE>
static void launch_pairwise(const typename PairArgsOf<MODE>::type& a, hipStream_t st, unsigned grid_y = 1) {
  const bool vec = a.D % 4 == 0 && ((uintptr_t)a.u & 15) == 0 && ((uintptr_t)a.v & 15) == 0;
  const unsigned grid = cdiv(a.M, PW_BM) * a.nsplit;
  if (vec) hipLaunchKernelGGL((pairwise_kernel<MODE, true>), dim3(grid, grid_y), dim3(PW_NT), 0, st, a);
  else hipLaunchKernelGGL((pairwise_kernel<MODE, false>), dim3(grid, grid_y), dim3(PW_NT), 0, st, a);
}

static bool pair_sizes_ok(long M, long N, long D) {
  return M > 0 && N > 0 && D > 0 && M * D < (1L << 40) && N * D < (1L << 40) && M < (1L << 30) && N < (1L << 30);
}

extern "C" int ldmae_pairwise_logits(const float* u, int M, int D, const float* w, int N, float* out, void* stream) {
  LDMAE_REQUIRE(u && w && out && pair_sizes_ok(M, N, D), "pairwise_logits: bad arguments (M %d, N %d, D %d)", M, N, D);
  const int col_tiles = (int)cdiv(N, PW_BN);
  PairArgs a{u, w, nullptr, nullptr, nullptr, nullptr, M, N, D, col_tiles, 1, 0, out, nullptr, nullptr};
  launch_pairwise<PW_LOGITS>(a, as_stream(stream));
  LDMAE_CHECK_LAUNCH("pairwise_logits");
  return 0;
}

extern "C" long ldmae_knn_partials_bytes(int M, int nsplit) {
  if (M <= 0 || nsplit <= 0) return -1;
  return (long)M * nsplit * 2 * KNN_KP * (long)sizeof(float);
}

// merge: one thread per row, the KNN_KP smallest of its nparts partial lists (ascending), then radii[m, t] = list[nhood[t]]
struct Nhood { int k[PR_MAXK]; };

__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part, int M, int nparts, Nhood nh, int nk, float* __restrict__ radii) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float best[KNN_KP];
#pragma unroll
  for (int q = 0; q < KNN_KP; ++q) best[q] = INFINITY;
  const float* p = part + (size_t)m * nparts * KNN_KP;
  for (int e = 0; e < nparts * KNN_KP; ++e) {
    const float v = p[e];
    if (v < best[KNN_KP - 1]) {
#pragma unroll
      for (int q = KNN_KP - 1; q > 0; --q) best[q] = v < best[q - 1] ? best[q - 1] : (v < best[q] ? v : best[q]);
      best[0] = fminf(best[0], v);
    }
  }
#pragma unroll
  for (int t = 0; t < PR_MAXK; ++t) {
    if (t >= nk) break;
    float r = best[0];
#pragma unroll
    for (int q = 1; q < KNN_KP; ++q) r = nh.k[t] == q ? best[q] : r;     // register index by comparison (no scratch)
    radii[(size_t)m * nk + t] = r;
  }
}

extern "C" int ldmae_knn_radii(const float* x, const float* norms, int N, int D, const int* nhood, int nk, int nsplit, float* partials, float* radii,
                               void* stream) {
  LDMAE_REQUIRE(x && norms && nhood && partials && radii && pair_sizes_ok(N, N, D), "knn_radii: bad arguments (N %d, D %d)", N, D);
  LDMAE_REQUIRE(nk >= 1 && nk <= PR_MAXK && nsplit >= 1, "knn_radii: %d neighbourhood sizes (1..%d), nsplit %d (>= 1)", nk, PR_MAXK, nsplit);
  Nhood nh{};
  int kmax = 0;
  for (int t = 0; t < nk; ++t) {
    LDMAE_REQUIRE(nhood[t] >= 0 && nhood[t] < KNN_KP, "knn_radii: neighbourhood size %d outside [0, %d]", nhood[t], KNN_KP - 1);
    nh.k[t] = nhood[t];
    kmax = max(kmax, nhood[t]);
  }
  LDMAE_REQUIRE(N > kmax, "knn_radii: %d rows hold no %d-th nearest neighbour", N, kmax);
  const int col_tiles = (int)cdiv(N, PW_BN);
  const int tps = (col_tiles + nsplit - 1) / nsplit;
  PairArgs a{x, x, norms, norms, nullptr, nullptr, N, N, D, nsplit, tps, nk, partials, nullptr, nullptr};
  launch_pairwise<PW_KNN>(a, as_stream(stream));        // splits past the last column tile write +inf lists
  hipLaunchKernelGGL(knn_merge_kernel, dim3(cdiv(N, 256)), dim3(256), 0, as_stream(stream), partials, N, nsplit * 2, nh, nk, radii);
  LDMAE_CHECK_LAUNCH("knn_radii");
  return 0;
}

extern "C" int ldmae_pr_flags(const float* u, const float* nu, const float* ru, int M, const float* v, const float* nv, const float* rv, int N, int D,
                              int nk, int nsplit, int* u_in, int* v_in, void* stream) {
  LDMAE_REQUIRE(u && nu && ru && v && nv && rv && u_in && v_in && pair_sizes_ok(M, N, D), "pr_flags: bad arguments (M %d, N %d, D %d)", M, N, D);
  LDMAE_REQUIRE(nk >= 1 && nk <= PR_MAXK && nsplit >= 1, "pr_flags: %d neighbourhood sizes (1..%d), nsplit %d (>= 1)", nk, PR_MAXK, nsplit);
  const int col_tiles = (int)cdiv(N, PW_BN);
  const int tps = (col_tiles + nsplit - 1) / nsplit;
  PairArgs a{u, v, nu, nv, ru, rv, M, N, D, nsplit, tps, nk, nullptr, u_in, v_in};
  launch_pairwise<PW_PR>(a, as_stream(stream));
  LDMAE_CHECK_LAUNCH("pr_flags");
  return 0;
}

// ------------------------------------------------------------------------------------------------ ball counts (density / coverage)
extern "C" long ldmae_ball_counts_partials_bytes(int M, int nsplit) {
  if (M <= 0 || nsplit <= 0) return -1;
  return (long)M * nsplit * 2 * (long)sizeof(int);
}

__global__ __launch_bounds__(256) void count_merge_kernel(const int* __restrict__ part, int M, int nparts, int* __restrict__ counts) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int* p = part + (size_t)m * nparts;
  int c = 0;
  for (int e = 0; e < nparts; ++e) c += p[e];
  counts[m] = c;
}

extern "C" int ldmae_ball_counts(const float* u, const float* nu, const float* ru, int M, const float* v, const float* nv, int N, int D, int nsplit,
                                 int* partials, int* counts, void* stream) {
  LDMAE_REQUIRE(u && nu && ru && v && nv && partials && counts && pair_sizes_ok(M, N, D), "ball_counts: bad arguments (M %d, N %d, D %d)", M, N, D);
  LDMAE_REQUIRE(nsplit >= 1 && (long)M * nsplit < (1L << 30), "ball_counts: nsplit %d (>= 1, M * nsplit < 2^30)", nsplit);
  const int col_tiles = (int)cdiv(N, PW_BN);
  const int tps = (col_tiles + nsplit - 1) / nsplit;
  PairArgs a{u, v, nu, nv, ru, nullptr, M, N, D, nsplit, tps, 1, nullptr, partials, nullptr};
  launch_pairwise<PW_COUNT>(a, as_stream(stream));      // splits past the last column tile write zero counts
  hipLaunchKernelGGL(count_merge_kernel, dim3(cdiv(M, 256)), dim3(256), 0, as_stream(stream), partials, M, nsplit * 2, counts);
  LDMAE_CHECK_LAUNCH("ball_counts");
  return 0;
}

// ------------------------------------------------------------------------------------------------ KID (polynomial-kernel sums)
extern "C" long ldmae_kid_workspace_bytes(int S, int m) {
  if (S <= 0 || m <= 0) return -1;
  return (long)S * 3 * cdiv(m, PW_BM) * cdiv(m, PW_BN) * (long)sizeof(double);
}

// out[s, which] = the tile partials of (s, which) added in ascending (row tile, column tile) order: one thread per sum
__global__ __launch_bounds__(256) void kid_fold_kernel(const double* __restrict__ part, int nsums, int tiles, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nsums) return;
  const double* p = part + (size_t)i * tiles;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += p[t];
  out[i] = s;
}

extern "C" int ldmae_kid_sums(const float* a, int Na, const float* b, int Nb, int D, const int* idx_a, const int* idx_b, int S, int m, float gamma,
                              float coef0, int nsplit, void* workspace, double* out, void* stream) {
  LDMAE_REQUIRE(a && b && idx_a && idx_b && workspace && out && pair_sizes_ok(Na, Nb, D), "kid_sums: bad arguments (Na %d, Nb %d, D %d)", Na, Nb, D);
  LDMAE_REQUIRE(S >= 1 && 3L * S <= 65535 && m >= 2 && m <= Na && m <= Nb && nsplit >= 1,
                "kid_sums: %d subsets (1..21845) of %d rows (2..min(Na, Nb) = %d), nsplit %d (>= 1)", S, m, Na < Nb ? Na : Nb, nsplit);
  const int row_tiles = (int)cdiv(m, PW_BM), col_tiles = (int)cdiv(m, PW_BN);
  const int tps = (col_tiles + nsplit - 1) / nsplit;
  KidArgs p{{a, b, nullptr, nullptr, nullptr, nullptr, m, m, D, nsplit, tps, 0, nullptr, nullptr, nullptr}, idx_a, idx_b, (double*)workspace, gamma, coef0};
  launch_pairwise<PW_KID>(p, as_stream(stream), 3u * S);      // every (row tile, column tile) is written: nsplit * tps >= column tiles
  hipLaunchKernelGGL(kid_fold_kernel, dim3(cdiv(3L * S, 256)), dim3(256), 0, as_stream(stream), (const double*)workspace, 3 * S, row_tiles * col_tiles,
                     out);
  LDMAE_CHECK_LAUNCH("kid_sums");
  return 0;
}

// ------------------------------------------------------------------------------------------------ softmax + Inception Score sums
// p = softmax(logits) per row in f32 (max-shifted, as TF's Softmax); h[i] = sum_c p log p in f64 with 0 log 0 := 0 (numpy's p * log(p) would
// give NaN there); S[s, c] = sum over the rows of split s of p[i, c] in f64, summed over fixed 128-row chunks and then over the chunks in
// order: bitwise reproducible, no atomics.
constexpr int IS_CHUNK = 128;

__global__ __launch_bounds__(256) void is_softmax_kernel(const float* __restrict__ logits, int C, float* __restrict__ probs, double* __restrict__ h) {
  __shared__ float redf[4];
  __shared__ double redd[4];
  const size_t row = blockIdx.x;
  const float* x = logits + row * C;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < C; c += 256) mx = fmaxf(mx, x[c]);
  mx = block_max(mx, redf);
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += expf(x[c] - mx);
  s = block_sum(s, redf);
  double hp = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float p = expf(x[c] - mx) / s;
    probs[row * C + c] = p;
    if (p > 0.f) hp += (double)p * log((double)p);
  }
  hp = block_sum(hp, redd);
  if (threadIdx.x == 0) h[row] = hp;
}

// chunk (s, q): rows [s * split + q * CHUNK, min(+CHUNK, end of split s, M)); one thread per column
__global__ __launch_bounds__(256) void is_colsum_chunk_kernel(const float* __restrict__ probs, int M, int C, int split, int cps,
                                                              double* __restrict__ ws) {
  const int c = blockIdx.x * 256 + threadIdx.x, chunk = blockIdx.y;
  if (c >= C) return;
  const int s = chunk / cps, q = chunk % cps;
  const long r0 = (long)s * split + (long)q * IS_CHUNK;
  const long r1 = min(min(r0 + IS_CHUNK, (long)s * split + split), (long)M);
  double acc = 0.0;
  for (long r = r0; r < r1; ++r) acc += (double)probs[r * C + c];
  ws[(size_t)chunk * C + c] = acc;
}

__global__ __launch_bounds__(256) void is_colsum_final_kernel(const double* __restrict__ ws, int C, int nsplit, int cps, double* __restrict__ S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nsplit * C) return;
  const int c = (int)(i % C), s = (int)(i / C);
  double acc = 0.0;
  for (int q = 0; q < cps; ++q) acc += ws[((size_t)s * cps + q) * C + c];
  S[i] = acc;
}

static long is_probs_bytes(int M, int C) { return ((long)M * C * (long)sizeof(float) + 255) / 256 * 256; }

extern "C" long ldmae_adm_is_workspace_bytes(int M, int C, int split) {
  if (M <= 0 || C <= 0 || split <= 0) return -1;
  const long nsplit = cdiv(M, split), cps = cdiv(split, IS_CHUNK);
  return is_probs_bytes(M, C) + nsplit * cps * C * (long)sizeof(double);
}

extern "C" int ldmae_adm_softmax_is(const float* logits, int M, int C, int split, void* workspace, double* h, double* S, void* stream) {
  LDMAE_REQUIRE(logits && workspace && h && S && M > 0 && C > 0 && split > 0 && (long)M * C < (1L << 40), "adm_softmax_is: bad arguments");
  const int nsplit = (int)cdiv(M, split), cps = (int)cdiv(split, IS_CHUNK);
  LDMAE_REQUIRE((long)nsplit * cps < 65536, "adm_softmax_is: %d splits of %d rows is too many chunks", nsplit, split);
  float* probs = (float*)workspace;
  double* ws = (double*)((char*)workspace + is_probs_bytes(M, C));
  hipLaunchKernelGGL(is_softmax_kernel, dim3(M), dim3(256), 0, as_stream(stream), logits, C, probs, h);
  hipLaunchKernelGGL(is_colsum_chunk_kernel, dim3(cdiv(C, 256), nsplit * cps), dim3(256), 0, as_stream(stream), probs, M, C, split, cps, ws);
  hipLaunchKernelGGL(is_colsum_final_kernel, dim3(cdiv((long)nsplit * C, 256)), dim3(256), 0, as_stream(stream), ws, C, nsplit, cps, S);
  LDMAE_CHECK_LAUNCH("adm_softmax_is");
  return 0;
}
