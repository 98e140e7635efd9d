// Dispersive Loss on one block's features (transport.Transport(dispersive=...)): L = log mean_ij exp(-||z_i - z_j||^2 / (K tau)) of z [B, K] f32
// and its gradient dz = g C z.  The contract is in include/ldmae_hip.h; DESIGN.md section 28 has the layout, the split plan and the bounds.
//
// Both products run on v_mfma_f32_32x32x2_f32 with exact f32 operands (the Gram form n_i + n_j - 2 G_ij cancels: bf16 operands are out).
//   forward   gram:    block (tile pair p, slab s) forms the 128 x 128 tile (ti <= tj) of z z^T over the K-slab s into P[s]; wave (wr, wc) owns
//                      64 x 64 of it as 2 x 2 MFMA tiles, and in a diagonal pair the wave below the diagonal (wr > wc) computes nothing.
//             reduce:  G[i][j] = P[0][i][j] + P[1][i][j] + ... in slab order for every 64-tile on or above the diagonal, mirrored below it.
//             rowsum:  block i: r_i = sum_j e_ij in f64 (thread t adds j = t, t + 256, ... in order, then block_sum).
//             finish:  block i: S = sum r (the same f64 order in every block), row i of C; block 0 writes L.
//   backward  block (column slab c, row band b) forms dz[256 b .. , 64 c .. ] = g * (C z): one writer per element, j ascending.
// No atomics: every sum has one fixed order that depends on (B, K) alone, so two calls give the same bits.
//
// k order inside the MFMA chains.  A group of 8 consecutive k (forward: columns of z, backward: rows j of z) is read as one float4 per lane
// half h = lane >> 5 (k = 8 q + 4 h + e, e = 0 .. 3), and MFMA number e of the group multiplies element e of both operands: the chain visits
// k = 8q, 8q + 4, 8q + 1, 8q + 5, ... .  The order is the same for every output element.
#include "flat_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_TILE = 128;                 // rows / columns of G per block (forward)
constexpr int GR_BK = 64;                    // forward: k per LDS stage -- 256 contiguous bytes of every row per stage
constexpr int GR_LD = GR_BK + 4;             // LDS row stride in floats: 16-byte rows, 16 consecutive rows on 16 distinct 4-bank slots
constexpr int DP_BK = 32;                    // backward: rows j of z per LDS stage
constexpr int DP_LD = DP_BK + 4;
constexpr long DP_MIN_SLAB = 1024;           // shortest K-slab
constexpr long DP_TARGET_BLOCKS = 512;       // the split aims at this many gram blocks (two per CU)
constexpr int DP_BM = 256;                   // backward: rows of dz per block
constexpr int DP_BN = 64;                    // backward: columns of dz per block
constexpr int DP_ZLD = DP_BN + 4;

struct Plan {
  int tiles, pairs, slabs;
  long slab;                                 // slab length, a multiple of GR_BK
};

inline Plan make_plan(int B, long K) {
  Plan p;
  p.tiles = (B + DP_TILE - 1) / DP_TILE;
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  long want = (K * p.pairs + DP_TARGET_BLOCKS - 1) / DP_TARGET_BLOCKS;
  want = (want + GR_BK - 1) / GR_BK * GR_BK;
  p.slab = want > DP_MIN_SLAB ? want : DP_MIN_SLAB;
  p.slabs = (int)((K + p.slab - 1) / p.slab);
  return p;
}

// workspace: r [B] f64 | G [B, B] f32 | P [slabs, B, B] f32
inline size_t ws_r_bytes(int B) { return ((size_t)B * 8 + 15) & ~(size_t)15; }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---------------------------------------------------------------- forward: partial Gram tiles
__global__ __launch_bounds__(DP_THREADS) void disp_gram_kernel(const float* __restrict__ z, float* __restrict__ P, int B, long K, long slab, int tiles) {
  __shared__ __attribute__((aligned(16))) float lds[2 * DP_TILE * GR_LD];
  float* As = lds;
  // pair index -> (ti <= tj); the pairs of one slab are neighbours in the grid, so they run together and the second reader of a row finds it
  // in the Infinity Cache
  int ti = 0, rest = blockIdx.x;
  while (rest >= tiles - ti) { rest -= tiles - ti; ++ti; }
  const int tj = ti + rest;
  const bool diag = ti == tj;
  float* Bs = diag ? As : lds + DP_TILE * GR_LD;
  const int i0 = ti * DP_TILE, j0 = tj * DP_TILE;
  const long kbeg = (long)blockIdx.y * slab;
  const long kend = kbeg + slab < K ? kbeg + slab : K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const bool idle = diag && wr > wc;                       // its tile is the mirror image of wave (0, 1)'s
  const int lr = lane & 31, lh = lane >> 5;

  // stage: thread t brings the float4s f = t, t + 256, ..., t + 1792 of each 128 x 64 tile: row f / 16, columns 4 (f % 16) ..
  float4 ra[8], rb[8];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = tid + u * DP_THREADS, row = f >> 4;
      const long k = k0 + ((f & 15) << 2);
      const bool in = k < kend;                            // K % 4 == 0 and slabs start on multiples of 64: a float4 is all in or all out
      ra[u] = (in && i0 + row < B) ? *(const float4*)(z + (long)(i0 + row) * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (!diag) rb[u] = (in && j0 + row < B) ? *(const float4*)(z + (long)(j0 + row) * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

  fetch(kbeg);
  for (long k0 = kbeg; k0 < kend; k0 += GR_BK) {
    __syncthreads();                                       // the previous stage's fragment reads are done
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = tid + u * DP_THREADS, row = f >> 4, c = (f & 15) << 2;
      *(float4*)(As + row * GR_LD + c) = ra[u];
      if (!diag) *(float4*)(Bs + row * GR_LD + c) = rb[u];
    }
    __syncthreads();
    if (k0 + GR_BK < kend) fetch(k0 + GR_BK);              // in flight under the MFMAs
    if (!idle) {
#pragma unroll
      for (int q = 0; q < GR_BK / 8; ++q) {
        float4 a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) a[m] = *(const float4*)(As + (wr * 64 + m * 32 + lr) * GR_LD + 8 * q + 4 * lh);
#pragma unroll
        for (int n = 0; n < 2; ++n) b[n] = *(const float4*)(Bs + (wc * 64 + n * 32 + lr) * GR_LD + 8 * q + 4 * lh);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            acc[m][n] = mfma32(a[m].x, b[n].x, acc[m][n]);
            acc[m][n] = mfma32(a[m].y, b[n].y, acc[m][n]);
            acc[m][n] = mfma32(a[m].z, b[n].z, acc[m][n]);
            acc[m][n] = mfma32(a[m].w, b[n].w, acc[m][n]);
          }
      }
    }
  }
  if (idle) return;
  // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* Ps = P + (long)blockIdx.y * B * B;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int gj = j0 + wc * 64 + n * 32 + lr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int gi = i0 + wr * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (gi < B && gj < B) Ps[(long)gi * B + gj] = acc[m][n][e];
      }
    }
}

// G = the partial tiles added in slab order; block (bi <= bj) owns the 64 x 64 tile the gram kernel's wave wrote
__global__ __launch_bounds__(DP_THREADS) void disp_reduce_kernel(const float* __restrict__ P, float* __restrict__ G, int B, int slabs) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const int j = bj * 64 + (threadIdx.x & 63);
  if (j >= B) return;
  const long BB = (long)B * B;
  for (int e = 0; e < 16; ++e) {
    const int i = bi * 64 + e * 4 + (threadIdx.x >> 6);
    if (i >= B) continue;
    const float* p = P + (long)i * B + j;
    float s = p[0];
    for (int sl = 1; sl < slabs; ++sl) s += p[sl * BB];
    G[(long)i * B + j] = s;
    if (bi != bj) G[(long)j * B + i] = s;
  }
}

__device__ __forceinline__ double disp_e(const float* __restrict__ G, int B, int i, int j, double ni, double kt) {
  if (i == j) return 1.0;                                  // d_ii = 0, set
  double d = ni + (double)G[(long)j * B + j] - 2.0 * (double)G[(long)i * B + j];
  d = d > 0.0 ? d : 0.0;
  return exp(-d / kt);
}

__global__ __launch_bounds__(DP_THREADS) void disp_rowsum_kernel(const float* __restrict__ G, double* __restrict__ r, int B, double kt) {
  __shared__ double slot[4];
  const int i = blockIdx.x;
  const double ni = (double)G[(long)i * B + i];
  double s = 0.0;
  for (int j = threadIdx.x; j < B; j += DP_THREADS) s += disp_e(G, B, i, j, ni, kt);
  s = block_sum(s, slot);
  if (threadIdx.x == 0) r[i] = s;
}

__global__ __launch_bounds__(DP_THREADS) void disp_finish_kernel(const float* __restrict__ G, const double* __restrict__ r, float* __restrict__ C,
                                                                  float* __restrict__ loss, int B, double kt) {
  __shared__ double slot[4];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int m = threadIdx.x; m < B; m += DP_THREADS) s += r[m];
  const double S = block_sum(s, slot);                     // the same order in every block: one S
  const double coef = 4.0 / (S * kt), ri = r[i], ni = (double)G[(long)i * B + i];
  for (int j = threadIdx.x; j < B; j += DP_THREADS) {
    const double e = disp_e(G, B, i, j, ni, kt);
    C[(long)i * B + j] = (float)(coef * (i == j ? e - ri : e));
  }
  if (i == 0 && threadIdx.x == 0) loss[0] = (float)log(S / ((double)B * (double)B));
}

// ---------------------------------------------------------------- backward: dz = g * (C z)
template <bool VEC>
__global__ __launch_bounds__(DP_THREADS) void disp_bwd_kernel(const float* __restrict__ C, const float* __restrict__ z, float* __restrict__ dz, int B, long K,
                                                               float g) {
  __shared__ __attribute__((aligned(16))) float lds[DP_BM * DP_LD + DP_BK * DP_ZLD];
  float* Cs = lds;                                         // [256 rows i][32 j]
  float* Zs = lds + DP_BM * DP_LD;                         // [32 j][64 columns]
  const long c0 = (long)blockIdx.x * DP_BN;
  const int i0 = blockIdx.y * DP_BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  float4 rc[8], rz[2];
  auto fetch = [&](int jb) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {                          // C tile: float4 f = t + 256 u: row f / 8, j = jb + 4 (f % 8) ..
      const int f = tid + u * DP_THREADS, i = i0 + (f >> 3), j = jb + ((f & 7) << 2);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < B) {
        const float* p = C + (long)i * B + j;
        if constexpr (VEC) {                               // B % 4 == 0: a float4 of a row is all in or all out, and 16-byte aligned
          if (j < B) v = *(const float4*)p;
        } else {
          if (j < B) v.x = p[0];
          if (j + 1 < B) v.y = p[1];
          if (j + 2 < B) v.z = p[2];
          if (j + 3 < B) v.w = p[3];
        }
      }
      rc[u] = v;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {                          // z tile: float4 f = t + 256 u: row jb + f / 16, columns c0 + 4 (f % 16) ..
      const int f = tid + u * DP_THREADS, j = jb + (f >> 4);
      const long c = c0 + ((f & 15) << 2);
      rz[u] = (j < B && c < K) ? *(const float4*)(z + (long)j * K + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

  fetch(0);
  for (int jb = 0; jb < B; jb += DP_BK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = tid + u * DP_THREADS;
      *(float4*)(Cs + (f >> 3) * DP_LD + ((f & 7) << 2)) = rc[u];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int f = tid + u * DP_THREADS;
      *(float4*)(Zs + (f >> 4) * DP_ZLD + ((f & 15) << 2)) = rz[u];
    }
    __syncthreads();
    if (jb + DP_BK < B) fetch(jb + DP_BK);
#pragma unroll
    for (int q = 0; q < DP_BK / 8; ++q) {
      float4 a[2];
      float b[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *(const float4*)(Cs + (wave * 64 + m * 32 + lr) * DP_LD + 8 * q + 4 * lh);
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) b[n][e] = Zs[(8 * q + 4 * lh + e) * DP_ZLD + n * 32 + lr];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          acc[m][n] = mfma32(a[m].x, b[n][0], acc[m][n]);
          acc[m][n] = mfma32(a[m].y, b[n][1], acc[m][n]);
          acc[m][n] = mfma32(a[m].z, b[n][2], acc[m][n]);
          acc[m][n] = mfma32(a[m].w, b[n][3], acc[m][n]);
        }
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const long c = c0 + n * 32 + lr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + wave * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (i < B && c < K) dz[(long)i * K + c] = g * acc[m][n][e];
      }
    }
}

inline int disp_check_shape(const char* op, int B, long K) {
  LDMAE_REQUIRE(B >= 1 && B <= 1024, "%s: B = %d samples, expected 1 .. 1024", op, B);
  LDMAE_REQUIRE(K >= 4 && K % 4 == 0, "%s: K = %ld features per sample, expected a positive multiple of 4 (16-byte accesses)", op, K);
  LDMAE_REQUIRE((long)B * K <= 0x7fffffffL * 4, "%s: B K = %ld elements is too large", op, (long)B * K);
  return LDMAE_OK;
}

}  // namespace

extern "C" int ldmae_dispersive_slabs(int B, long K) {
  if (disp_check_shape("dispersive_slabs", B, K) != LDMAE_OK) return -1;
  return make_plan(B, K).slabs;
}

extern "C" long ldmae_dispersive_workspace_bytes(int B, long K) {
  if (disp_check_shape("dispersive_workspace_bytes", B, K) != LDMAE_OK) return -1;
  const Plan p = make_plan(B, K);
  return (long)(ws_r_bytes(B) + ((size_t)p.slabs + 1) * B * B * 4);
}

extern "C" int ldmae_dispersive_fwd(const float* z, float* loss, float* C, int B, long K, float tau, void* workspace, void* stream) {
  if (int rc = disp_check_shape("dispersive_fwd", B, K)) return rc;
  LDMAE_REQUIRE(z && loss && C && workspace, "dispersive_fwd: null pointer");
  LDMAE_REQUIRE(tau > 0.f && tau <= 3.4e38f, "dispersive_fwd: tau = %g, expected a finite value > 0", (double)tau);
  LDMAE_REQUIRE(is_aligned(z, 16) && is_aligned(C, 4) && is_aligned(loss, 4) && is_aligned(workspace, 16),
                "dispersive_fwd: z and the workspace must be 16-byte aligned, C and loss 4-byte aligned");
  const size_t zb = (size_t)B * K * 4, cb = (size_t)B * B * 4, wb = (size_t)ldmae_dispersive_workspace_bytes(B, K);
  LDMAE_REQUIRE(disjoint(C, cb, z, zb) && disjoint(loss, 4, z, zb) && disjoint(loss, 4, C, cb), "dispersive_fwd: z, C and loss must not overlap");
  LDMAE_REQUIRE(disjoint(workspace, wb, z, zb) && disjoint(workspace, wb, C, cb) && disjoint(workspace, wb, loss, 4),
                "dispersive_fwd: the workspace overlaps an operand");
  const Plan p = make_plan(B, K);
  double* r = (double*)workspace;
  float* G = (float*)((char*)workspace + ws_r_bytes(B));
  float* P = G + (size_t)B * B;
  const double kt = (double)K * (double)tau;
  hipStream_t st = as_stream(stream);
  const unsigned t64 = cdiv(B, 64);
  hipLaunchKernelGGL(disp_gram_kernel, dim3((unsigned)p.pairs, (unsigned)p.slabs), dim3(DP_THREADS), 0, st, z, P, B, K, p.slab, p.tiles);
  hipLaunchKernelGGL(disp_reduce_kernel, dim3(t64, t64), dim3(DP_THREADS), 0, st, (const float*)P, G, B, p.slabs);
  hipLaunchKernelGGL(disp_rowsum_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, st, (const float*)G, r, B, kt);
  hipLaunchKernelGGL(disp_finish_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, st, (const float*)G, (const double*)r, C, loss, B, kt);
  LDMAE_CHECK_LAUNCH("dispersive_fwd");
  return LDMAE_OK;
}

extern "C" int ldmae_dispersive_bwd(const float* C, const float* z, float g, float* dz, int B, long K, void* stream) {
  if (int rc = disp_check_shape("dispersive_bwd", B, K)) return rc;
  LDMAE_REQUIRE(C && z && dz, "dispersive_bwd: null pointer");
  LDMAE_REQUIRE(is_aligned(z, 16) && is_aligned(dz, 16) && is_aligned(C, 4), "dispersive_bwd: z and dz must be 16-byte aligned, C 4-byte aligned");
  const size_t zb = (size_t)B * K * 4, cb = (size_t)B * B * 4;
  LDMAE_REQUIRE(disjoint(dz, zb, z, zb) && disjoint(dz, zb, C, cb), "dispersive_bwd: dz overlaps an input");
  hipStream_t st = as_stream(stream);
  const dim3 grid(cdiv(K, DP_BN), cdiv(B, DP_BM));
  if (B % 4 == 0 && is_aligned(C, 16)) hipLaunchKernelGGL(disp_bwd_kernel<true>, grid, dim3(DP_THREADS), 0, st, C, z, dz, B, K, g);
  else hipLaunchKernelGGL(disp_bwd_kernel<false>, grid, dim3(DP_THREADS), 0, st, C, z, dz, B, K, g);
  LDMAE_CHECK_LAUNCH("dispersive_bwd");
  return LDMAE_OK;
}
