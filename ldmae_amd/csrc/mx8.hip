// MXFP8 sampling mode (contract in include/ldmae_hip.h): the MX block quantiser, the RMSNorm + modulate pass that
// quantises its own output, and the block-scaled fp8 NT GEMM on v_mfma_scale_f32_16x16x128_f8f6f4 with the epilogues of gemm_nt_common.h.
//
// The GEMM is gemm_nt_lines_kernel (gemm_nt_lines.hip) with one-byte elements: a 128-B LDS row is 128 k, so a half-block slot (256 rows x
// 128 B) is ONE 128-deep K-step.  Ring, issue stream (A0 B0 A1 B1 ..., slot = position mod 5), counted waits, the stagger of the two wave
// groups, XCD tile ownership and the epilogue scratch placement are that kernel's.  A K-step is multiplied in four barrier quarters: quarter h
// covers accumulator rows 4 (h >> 1) .. +3 and columns 2 (h & 1) .. +1 of the wave's 8 x 4 MFMA tiles (8 scaled MFMAs; 48 fragment registers
// live, as in the bf16 kernel -- two phases of 16 MFMAs spilled).
// Operand lane map of the scaled MFMA, MEASURED (a one-hot / power-of-two probe through this kernel, then pinned by the exact-integer test
// of tests/test_gpu_mx8.py): with g = lane >> 4, registers 0-3 of a lane's operand hold k = 16 g .. 16 g + 15 of row (lane & 15) and
// registers 4-7 hold k = 64 + 16 g .. 64 + 16 g + 15; the scale in byte 0 of lane (row, g)'s scale register multiplies k = 32 g .. 32 g + 31
// of that row -- the data of lane groups 2 (g & 1) and 2 (g & 1) + 1, register half g >> 1 -- so lane (row, g) supplies the E8M0 byte of
// (row, 32-block g).  (32 contiguous k per lane, the first guess, is exact with unit scales and multiplies every 16-chunk c by the scale of
// block 2 (c & 1) + (c >> 2) otherwise.)  The 128 products of one instruction are NOT summed in f32: worst error 3.5e-4 of sum |a| |w|
// (tests/mx8_check.py bounds it).
// The scale bytes are not staged: every lane reads the scale byte of its row and 32-block straight from global memory, half a K-step ahead
// (12 byte loads per lane and K-step; the compiler counts their waits, the ring DMA is invisible to it and can only be over-waited).
#include "rowwise_common.h"

#include "gemm_nt_common.h"

#include <atomic>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// ---------------------------------------------------------------- launch counts of this mode (separate from ldmae_launch_counts)
static std::atomic<long> g_mx8_counts[3];
static void mx8_count(int slot) { g_mx8_counts[slot].fetch_add(1, std::memory_order_relaxed); }
extern "C" int ldmae_mx8_launch_counts(long* counts, int n, int reset) {
  LDMAE_REQUIRE(counts && n >= 0 && n <= 3, "mx8_launch_counts: counts null or n outside 0..3");
  for (int i = 0; i < n; ++i) counts[i] = g_mx8_counts[i].load(std::memory_order_relaxed);
  if (reset)
    for (auto& c : g_mx8_counts) c.store(0, std::memory_order_relaxed);
  return LDMAE_OK;
}

// ---------------------------------------------------------------- the quantiser
// scale exponent of a block from the bits of amax = m * 2^x (m in [1,2)): x - 8 for m <= 1.75, else x - 7 -- the smallest e with
// amax * 2^-e <= 448; clamped below at -127 (amax == 0 lands there by itself).  x <= 127, so e <= 120 and 2^-e is a normal float.
__device__ __forceinline__ int mx8_exponent(float amax) {
  const unsigned b = __builtin_bit_cast(unsigned, amax);
  const int e = (int)(b >> 23) - 127 - ((b & 0x7FFFFFu) <= 0x600000u ? 8 : 7);
  return max(e, -127);
}
__device__ __forceinline__ float mx8_inv_scale(int e) { return __builtin_bit_cast(float, (unsigned)(127 - e) << 23); }
// four floats (already multiplied by 2^-e: |v| <= 448) -> four OCP e4m3fn bytes, round to nearest even; element 0 in byte 0
__device__ __forceinline__ int mx8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}
template <int CTRL> __device__ __forceinline__ float dpp_max_f(float v) {      // v >= 0: the 0 of an out-of-row read is neutral
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true)));
}

// one pass: a thread owns 8 consecutive elements, four threads (a DPP quad) one 32-block.  n8 = M * K / 8 is a multiple of 4, so a quad is
// live as a whole; threads past the end repeat the last one's loads and store nothing.
template <typename T>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(const T* __restrict__ src, int ld, uint8_t* __restrict__ q, uint8_t* __restrict__ sc,
                                                           long n8, int K) {
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = t0 < n8;
  const long t = live ? t0 : n8 - 1;
  const int k8 = K >> 3;
  const long row = t / k8;
  const int c = (int)(t - row * k8) * 8;
  float v[8];
  Vec8<T>::load(src + (size_t)row * ld + c, v);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = dpp_max_f<0xB1>(amax);            // quad_perm [1,0,3,2]
  amax = dpp_max_f<0x4E>(amax);            // quad_perm [2,3,0,1]
  const int e = mx8_exponent(amax);
  const float is = mx8_inv_scale(e);
  if (!live) return;
  i32x2 o;
  o[0] = mx8_pack4(v[0] * is, v[1] * is, v[2] * is, v[3] * is);
  o[1] = mx8_pack4(v[4] * is, v[5] * is, v[6] * is, v[7] * is);
  *(i32x2*)(q + (size_t)row * K + c) = o;
  if ((threadIdx.x & 3) == 0) sc[(size_t)row * (K >> 5) + (c >> 5)] = (uint8_t)(e + 127);
}

extern "C" int ldmae_mx8_quantize(int src_dtype, const void* src, int ld, void* q, void* scales, int M, int K, void* stream) {
  LDMAE_REQUIRE(src_dtype == LDMAE_F32 || src_dtype == LDMAE_BF16, "mx8_quantize: source must be f32 or bf16, got dtype %d", src_dtype);
  LDMAE_REQUIRE(src && q && scales && M > 0 && K > 0, "mx8_quantize: null pointer or empty");
  LDMAE_REQUIRE(K % 128 == 0 && ld >= K && ld % 8 == 0, "mx8_quantize: K=%d must be a multiple of 128, ld=%d a multiple of 8 and >= K", K, ld);
  LDMAE_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)q & 7) == 0, "mx8_quantize: source must be 16-B aligned, q 8-B aligned");
  const long n8 = (long)M * K / 8;
  hipStream_t st = as_stream(stream);
  dtype_dispatch<float, bf16>(src_dtype, [&](auto t) {        // (codes outside the two were refused above)
    using T = tag_t<decltype(t)>;
    hipLaunchKernelGGL(mx8_quantize_kernel<T>, dim3(cdiv(n8, 256)), dim3(256), 0, st, (const T*)src, ld, (uint8_t*)q, (uint8_t*)scales, n8, K);
  });
  mx8_count(0);
  LDMAE_CHECK_LAUNCH("mx8_quantize");
  return LDMAE_OK;
}

// ---------------------------------------------------------------- RMSNorm + modulate + quantise
// The arithmetic of rmsnorm_mod_fwd_kernel<NCH, bf16> (elementwise.hip) up to and including its bf16 rounding, then the quantiser on the
// rounded values while they are in registers.  A lane holds 4 consecutive columns per 256-column chunk, so a 32-block is 8 lanes.

// quantise one 256-column chunk of a row from the modulated values: bf16 rounding, 8-lane amax, e4m3 bytes and the scale byte
__device__ __forceinline__ void mx8_norm_emit(float4 y, bool inr, int lane, uint8_t* __restrict__ qrow, uint8_t* __restrict__ srow, int c) {
  const float y0 = (float)(bf16)y.x, y1 = (float)(bf16)y.y, y2 = (float)(bf16)y.z, y3 = (float)(bf16)y.w;
  float amax = inr ? fmaxf(fmaxf(fabsf(y0), fabsf(y1)), fmaxf(fabsf(y2), fabsf(y3))) : 0.f;
  amax = dpp_max_f<0xB1>(amax);
  amax = dpp_max_f<0x4E>(amax);
  amax = dpp_max_f<0x141>(amax);         // row_half_mirror: the other quad of the 8-lane group
  const int e = mx8_exponent(amax);
  const float is = mx8_inv_scale(e);
  if (inr) {
    *(int*)(qrow + 4 * c) = mx8_pack4(y0 * is, y1 * is, y2 * is, y3 * is);
    if ((lane & 7) == 0) srow[c >> 3] = (uint8_t)(e + 127);
  }
}

// (norm_mod_rows.inc is the body of rmsnorm_mod_fwd_kernel, `center` path included: the compiler's contraction choices in the sum of squares
// depend on it.  Only what becomes of the modulated values differs: NORM_EMIT hands them, with their float4 chunk index, to the quantiser)
template <int NCH, bool FULL = false>
__global__ __launch_bounds__(256) void rmsnorm_mod_fwd_mx8_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ shift, const float* __restrict__ scale,
                                                              int mod_ld, uint8_t* __restrict__ q, uint8_t* __restrict__ sc, float* __restrict__ rstd, int M, int D,
                                                              int rpb, float eps, int center = 0) {
#define NORM_EMIT(m, a, b, y) mx8_norm_emit(y, true, lane, q + (size_t)(m) * D, sc + (size_t)(m) * (D >> 5), ((a) + (b)) >> 2)
#include "norm_mod_rows.inc"
#undef NORM_EMIT
}

extern "C" int ldmae_rmsnorm_modulate_fwd_mx8(const float* x, const float* w, const float* shift, const float* scale, int mod_ld, void* q,
                                              void* scales, float* rstd, int M, int D, int rows_per_batch, float eps, void* stream) {
  LDMAE_REQUIRE(x && w && q && scales && M > 0 && D > 0, "rmsnorm_modulate_fwd_mx8: null pointer or empty");
  LDMAE_REQUIRE(D % 128 == 0 && D <= 2048 && (mod_ld % 4 == 0 || (!shift && !scale)), "rmsnorm_modulate_fwd_mx8: D=%d must be a multiple of 128 up to 2048, mod_ld=%d of 4", D, mod_ld);
  LDMAE_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0, "rmsnorm_modulate_fwd_mx8: M=%d %% rows_per_batch=%d != 0", M, rows_per_batch);
  LDMAE_REQUIRE(((uintptr_t)q & 3) == 0, "rmsnorm_modulate_fwd_mx8: q must be 4-B aligned");
  hipStream_t st = as_stream(stream);
  const unsigned grid = cdiv(M, 16);
  // the same choice of form as ldmae_rmsnorm_modulate_fwd makes for a bf16 output
  const bool full = D % 256 == 0 && M % 16 == 0 && rows_per_batch % 16 == 0;
  if (int e = row_nch_dispatch(D, [&](auto nch) {
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, x, w, shift, scale, mod_ld, (uint8_t*)q, (uint8_t*)scales, rstd, M, D, rows_per_batch, eps, 0); };
        if (full) launch(rmsnorm_mod_fwd_mx8_kernel<decltype(nch)::value, true>); else launch(rmsnorm_mod_fwd_mx8_kernel<decltype(nch)::value, false>);
      })) return e;
  mx8_count(1);
  LDMAE_CHECK_LAUNCH("rmsnorm_modulate_fwd_mx8");
  return LDMAE_OK;
}

// ---------------------------------------------------------------- the GEMM
#define MX8_BAR() do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); } while (0)

// A [M, lda] / B [N, ldb]: e4m3 bytes; As [M, K/32] / Bs [N, K/32]: E8M0 bytes, dense.  lda, ldb in bytes.
template <int EPI, typename OutT>
__global__ __launch_bounds__(512) void gemm_nt_mx8_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ As, const uint8_t* __restrict__ B,
                                                          const uint8_t* __restrict__ Bs, int M, int N, int K, int lda, int ldb, EpiArgs e, int ntiles) {
  constexpr int BM = 256, BN = 256, WN = 4, TM = 128, TNn = 64, MI = 8, NI = 4, SLOT = 256 * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (N + BN - 1) / BN;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_PTR(void, smem));
  // tile ownership as in gemm_nt_lines_kernel
  const bool persistent = (int)gridDim.x != ntiles;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
  const int rbx = (((M + BM - 1) / BM) + 7) / 8;
  const int first = persistent ? xcd * rbx * tiles_n + slot : (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tend = persistent ? min(ntiles, (xcd + 1) * rbx * tiles_n) : ntiles;
  const int tstride = persistent ? per_xcd : ntiles;
  const int nb = K / 128, ks = K >> 5;                       // K-steps; scale bytes per row

  // ---- ring DMA: the pieces, lane offsets and swizzle of gemm_nt_lines_kernel with one-byte elements
  const unsigned swz = (unsigned)(((lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7)) << 4);
  const unsigned voffA = (unsigned)(lane >> 3) * (unsigned)lda + swz, voffB = (unsigned)(lane >> 3) * (unsigned)ldb + swz;
  const char* pa[4];
  const char* pb[4];
  auto rowsA = [&](int t) {
    const int m0 = (t / tiles_n) * BM;
#pragma unroll
    for (int i = 0; i < 4; ++i) pa[i] = (const char*)(A + (size_t)min(m0 + 8 * wave + 64 * i, M - 8) * lda);
  };
  auto rowsB = [&](int t) {
    const int n0 = (t % tiles_n) * BN;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int brow = n0 + 8 * wave + 64 * i;
      // SwiGLU: tile row rl of B is w12 row ((rl & 32) ? Hs : 0) + n0 / 2 + (rl >> 6) * 32 + (rl & 31), as in gemm_nt_lines_kernel
      if constexpr (EPI == LDMAE_EPI_SWIGLU) brow = ((wave & 4) ? (N >> 1) : 0) + (n0 >> 1) + i * 32 + 8 * (wave & 3);
      pb[i] = (const char*)(B + (size_t)min(brow, N - 8) * ldb);
    }
  };
  int tA = first, jA = 0, tB = first, jB = 0;
  unsigned sA = 0, sB = 1;
  auto issueA = [&]() -> bool {
    if (tA >= tend) return false;
    const unsigned la = lds0 + sA * SLOT + wave * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16_s(pa[i] + jA * 128, voffA, la + i * 8192);
    sA = sA >= 3 ? sA - 3 : sA + 2;
    if (++jA == nb) { jA = 0; tA += tstride; if (tA < tend) rowsA(tA); }
    return true;
  };
  auto issueB = [&]() -> bool {
    if (tB >= tend) return false;
    const unsigned la = lds0 + sB * SLOT + wave * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16_s(pb[i] + jB * 128, voffB, la + i * 8192);
    sB = sB >= 3 ? sB - 3 : sB + 2;
    if (++jB == nb) { jB = 0; tB += tstride; if (tB < tend) rowsB(tB); }
    return true;
  };
  // fragment addresses inside a slot: row (lane & 15) of an MFMA tile; registers 0-3 of the operand are the 16 k bytes 16 g .. (16-B chunk g
  // = lane >> 4, at position g ^ s, s = (row >> 1) & 7), registers 4-7 the bytes 64 + 16 g .. (chunk g + 4: the same address with bit 6 flipped)
  const int fsw = ((lane >> 4) ^ ((lane & 15) >> 1)) << 4;
  const int a_off = (wm * TM + (lane & 15)) * 128 + fsw, b_off = (wn * TNn + (lane & 15)) * 128 + fsw;
  const int sbyte = lane >> 4;                              // this lane's byte of a K-step's four scale bytes
  const bool grpB = wm >= 1;

  int t = first;
  if (t < tend) {
    rowsA(t); rowsB(t);
    issueA(); issueB();
  }
  unsigned ga = 0, gb = 1;
  while (t < tend) {
    const int em0 = (t / tiles_n) * BM, en0 = (t % tiles_n) * BN;
    // Scale bytes of this lane's rows: A row of MFMA tile i, B row of tile jj (the SwiGLU interleave of rowsB); rows past the edge are
    // clamped (their products are never stored).  One byte load per (MFMA tile, K-step) at a 32-bit offset from the wave-uniform base;
    // the per-tile offsets are formed inside the K loop from one opaque register per operand (hoisted, they cost 12 registers and spilled).
    const unsigned abase = (unsigned)((em0 + wm * TM + (lane & 15)) * ks + sbyte), alim = (unsigned)((M - 1) * ks + sbyte);
    const unsigned bbase = (unsigned)(((EPI == LDMAE_EPI_SWIGLU ? (en0 >> 1) + wn * 32 : en0 + wn * TNn) + (lane & 15)) * ks + sbyte);
    const unsigned blim = (unsigned)((N - 1) * ks + sbyte);
    auto ld_a = [&](int i, int j) {
      unsigned ab = abase;
      asm volatile("" : "+v"(ab));
      return (int)As[min(ab + (unsigned)(16 * i * ks), alim) + (unsigned)(4 * j)];
    };
    auto ld_b = [&](int jj, int j) {
      unsigned bb = bbase;
      asm volatile("" : "+v"(bb));
      const int rr = EPI == LDMAE_EPI_SWIGLU ? ((jj & 2) ? (N >> 1) : 0) + (jj & 1) * 16 : 16 * jj;
      return (int)Bs[min(bb + (unsigned)(rr * ks), blim) + (unsigned)(4 * j)];
    };
    // sca[0..3] / scb: this K-step's; sca[4..7] are loaded in quarter 0 for quarter 2, sca[0..3] of the next K-step in quarter 1, scn (the
    // next K-step's B scales) in quarter 0 -- never between a ring DMA issue and the counted wait that follows it
    int sca[MI], scb[NI], scn[NI];
#pragma unroll
    for (int i = 0; i < MI / 2; ++i) sca[i] = ld_a(i, 0);
#pragma unroll
    for (int jj = 0; jj < NI; ++jj) scb[jj] = ld_b(jj, 0);
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_waitcnt(0x0F70);
    MX8_BAR();
    if (grpB) MX8_BAR();
    for (int j = 0; j < nb; ++j) {
      const char* sa = smem + ga * SLOT;
      const char* sb = smem + gb * SLOT;
      i32x8 af[MI / 2];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int ia = 4 * (h >> 1), ib = 2 * (h & 1);
        i32x8 bfr[NI / 2];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int jj = 0; jj < NI / 2; ++jj) {
          const int o = (ib + jj) * 2048;
          const i32x4 lo = *(const i32x4*)(sb + b_off + o), hi = *(const i32x4*)(sb + (b_off ^ 64) + o);
          bfr[jj] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
        if ((h & 1) == 0) {
#pragma unroll
          for (int i = 0; i < MI / 2; ++i) {
            const int o = (ia + i) * 2048;
            const i32x4 lo = *(const i32x4*)(sa + a_off + o), hi = *(const i32x4*)(sa + (a_off ^ 64) + o);
            af[i] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          }
        }
        if (h == 0) {
#pragma unroll
          for (int i = MI / 2; i < MI; ++i) sca[i] = ld_a(i, j);
          if (j + 1 < nb) {
#pragma unroll
            for (int jj = 0; jj < NI; ++jj) scn[jj] = ld_b(jj, j + 1);
          }
        }
        bool issued = false;
        if (h == 0) {
          if (j == 0) issueA();                           // the half-block deferred over the tile boundary
          issueB();
        } else if (h == 3 && j + 1 < nb) issued = issueA();
        __builtin_amdgcn_s_setprio(0);
        // block j+1 has to be complete one phase before anyone reads it
        if (grpB && h == 3 && j + 1 < nb) {
          if (issued) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        MX8_BAR();
#pragma unroll
        for (int i = 0; i < MI / 2; ++i)
#pragma unroll
          for (int jj = 0; jj < NI / 2; ++jj)
            acc[ia + i][ib + jj] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bfr[jj], acc[ia + i][ib + jj], 0, 0, 0, sca[ia + i], 0, scb[ib + jj]);
        // a quarter's accumulators are next read a whole K-step later: without this pin the optimiser sinks all 32 MFMAs below the K-step's
        // last barrier (and keeps every fragment of the K-step live: 128 registers, spilled)
#pragma unroll
        for (int i = 0; i < MI / 2; ++i)
#pragma unroll
          for (int jj = 0; jj < NI / 2; ++jj) asm volatile("" : "+v"(acc[ia + i][ib + jj]));
        if (h == 1 && j + 1 < nb) {                       // sca[0..3] are dead: the next K-step's
#pragma unroll
          for (int i = 0; i < MI / 2; ++i) sca[i] = ld_a(i, j + 1);
        }
        if (!grpB && h == 3 && j + 1 < nb) {
          if (issued) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        MX8_BAR();
      }
      if (j + 1 < nb) {
#pragma unroll
        for (int jj = 0; jj < NI; ++jj) scb[jj] = scn[jj];
      }
      ga = ga >= 3 ? ga - 3 : ga + 2;
      gb = gb >= 3 ? gb - 3 : gb + 2;
    }
    if (!grpB) MX8_BAR();
    const unsigned sx = sA >= 3 ? sA - 3 : sA + 2;
    float* ew = (float*)(smem + ((wave & 4) ? sB : sA) * SLOT) + (wave & 3) * (16 * 68);
    float* ex = (float*)(smem + sx * SLOT) + wave * 1024;
    t += tstride;
    // the qkv epilogue addresses q2 / k2 by whole wave slices (one head, 128 rows of one sample): a slice past the edge has nothing to write
    // (3 * heads * 64 need not be a multiple of the tile width here)
    if (EPI == LDMAE_EPI_QKV_ROPE && (en0 + wn * TNn >= N || em0 + wm * TM >= M)) continue;
    nt_epilogue<EPI, OutT, TM, TNn, MI, NI>(acc, ew, ex, e, em0, en0, wm, wn, lane, M, N);
  }
}

static bool mx8_shape_ok(int epi, long M, int N, int K, int lda, int ldb) {
  if (M < 8 || N < 8 || M * (K >> 5) >= (1l << 31) || (long)N * (K >> 5) >= (1l << 31) || M % 8 != 0 || N % 8 != 0 || K <= 0 || K % 128 != 0 || lda % 128 != 0 || ldb % 128 != 0 || lda < K || ldb < K) return false;
  return !(epi == LDMAE_EPI_SWIGLU && N % 256 != 0);
}

template <typename OutT>
static int launch_mx8(int epi, const void* A, const void* As, const void* B, const void* Bs, int M, int N, int K, int lda, int ldb, const EpiArgs& e,
                      int tile_launch, hipStream_t st) {
  const NtGrid g = nt_grid(M, N, tile_launch != 0);
  auto go = [&](auto E) {
    nt_launch(gemm_nt_mx8_kernel<decltype(E)::value, OutT>, g.grid, 512, 5 * 256 * 128, st, A, As, B, Bs, M, N, K, lda, ldb, e, g.ntiles);
  };
  if constexpr (sizeof(OutT) == 2) return nt_epi_dispatch<LDMAE_EPI_BIAS, LDMAE_EPI_GATE_RES, LDMAE_EPI_SWIGLU, LDMAE_EPI_QKV_ROPE>(epi, go);
  else return nt_epi_dispatch<LDMAE_EPI_BIAS, LDMAE_EPI_GATE_RES>(epi, go);
}

extern "C" int ldmae_gemm_nt_mx8_ok(int M, int N, int K, int lda, int ldb) { return mx8_shape_ok(LDMAE_EPI_BIAS, M, N, K, lda, ldb) ? 1 : 0; }

extern "C" int ldmae_gemm_nt_mx8(int out_dtype, int epi, const void* Aq, const void* As, int lda, const void* Wq, const void* Ws, int ldb, void* C,
                                 int ldc, int M, int N, int K, const float* bias, const float* xin, float* xout, const float* gate, int gate_ld,
                                 int rows_per_batch, void* stream) {
  const int tile_launch = (epi & LDMAE_EPI_TILE_LAUNCH) != 0;
  epi &= ~LDMAE_EPI_TILE_LAUNCH;
  LDMAE_REQUIRE(out_dtype == LDMAE_F32 || out_dtype == LDMAE_BF16, "gemm_nt_mx8: bad out_dtype %d", out_dtype);
  LDMAE_REQUIRE(Aq && As && Wq && Ws, "gemm_nt_mx8: null operand");
  LDMAE_REQUIRE(mx8_shape_ok(epi, M, N, K, lda, ldb),
                "gemm_nt_mx8: shape outside the kernel (M=%d N=%d multiples of 8, K=%d lda=%d ldb=%d multiples of 128, SwiGLU: N %% 256 == 0)", M, N, K, lda, ldb);
  LDMAE_REQUIRE(((uintptr_t)Aq & 127) == 0 && ((uintptr_t)Wq & 127) == 0 && ((uintptr_t)As & 3) == 0 && ((uintptr_t)Ws & 3) == 0,
                "gemm_nt_mx8: element operands must start on 128-B lines, scale operands on 4 B");
  EpiArgs e{};
  e.C = C; e.bias = bias; e.ldc = ldc; e.beta = 0.f; e.f16_max = 65504.f;
  if (epi == LDMAE_EPI_BIAS) {
    LDMAE_REQUIRE(C && ldc >= N, "gemm_nt_mx8: C null or ldc < N");
  } else if (epi == LDMAE_EPI_GATE_RES) {
    LDMAE_REQUIRE(xin && xout && rows_per_batch > 0 && (!gate || gate_ld >= N), "gemm_nt_mx8: gated-residual epilogue needs xin/xout (gate optional)");
    LDMAE_REQUIRE(M % rows_per_batch == 0, "gemm_nt_mx8: M=%d not a multiple of rows_per_batch=%d", M, rows_per_batch);
    e.xin = xin; e.xout = xout; e.gate = gate; e.gate_ld = gate_ld; e.rows_per_batch = rows_per_batch;
  } else if (epi == LDMAE_EPI_SWIGLU) {
    LDMAE_REQUIRE(out_dtype == LDMAE_BF16, "gemm_nt_mx8: swiglu epilogue writes bf16");
    LDMAE_REQUIRE(xout && (!C || ldc == N), "gemm_nt_mx8: swiglu epilogue needs hid (xout); h12 (C, ldc = N) may be NULL");
    e.xout = xout;
  } else {
    LDMAE_FAIL(LDMAE_ERR_INVALID, "gemm_nt_mx8: epilogue %d is not built in this mode (bias, gated residual, swiglu)", epi);
  }
  hipStream_t st = as_stream(stream);
  const int ok = out_dtype == LDMAE_BF16 ? launch_mx8<bf16>(epi, Aq, As, Wq, Ws, M, N, K, lda, ldb, e, tile_launch, st)
                                         : launch_mx8<float>(epi, Aq, As, Wq, Ws, M, N, K, lda, ldb, e, tile_launch, st);
  LDMAE_REQUIRE(ok, "gemm_nt_mx8: no kernel for epilogue %d with out_dtype %d", epi, out_dtype);
  mx8_count(2);
  LDMAE_CHECK_LAUNCH("gemm_nt_mx8");
  return LDMAE_OK;
}

extern "C" int ldmae_gemm_nt_qkv_rope_mx8_ok(int B, int N, int H, int hd, int K, int lda, int ldb) {
  const long M = (long)B * N;
  return hd == 64 && B > 0 && N > 0 && H > 0 && M % 256 == 0 && M < (1l << 31) && N % 128 == 0 && K > 0 && K % 128 == 0 &&
         lda % 128 == 0 && ldb % 128 == 0 && lda >= K && ldb >= K;
}

extern "C" int ldmae_gemm_nt_qkv_rope_mx8(const void* Aq, const void* As, int lda, const void* Wq, const void* Ws, int ldb, const float* bias, void* qkv,
                                          void* q2, void* k2, const float* wq, const float* wk, const float* cos, const float* sin, int B, int N,
                                          int H, int hd, int K, float eps, int store_raw_qk, int tile_launch, void* stream) {
  LDMAE_REQUIRE(Aq && As && Wq && Ws && qkv && q2 && k2 && cos && sin, "gemm_nt_qkv_rope_mx8: null pointer (only bias and wq / wk may be NULL)");
  LDMAE_REQUIRE(!wq == !wk, "gemm_nt_qkv_rope_mx8: pass both QK-norm weights or neither (RoPE only)");
  LDMAE_REQUIRE(ldmae_gemm_nt_qkv_rope_mx8_ok(B, N, H, hd, K, lda, ldb),
                "gemm_nt_qkv_rope_mx8: shape outside the fused kernel (head_dim 64, B*N %% 256 == 0, N %% 128 == 0, K / lda / ldb %% 128 == 0): "
                "B=%d N=%d H=%d hd=%d K=%d lda=%d ldb=%d", B, N, H, hd, K, lda, ldb);
  LDMAE_REQUIRE(((uintptr_t)Aq & 127) == 0 && ((uintptr_t)Wq & 127) == 0 && ((uintptr_t)As & 3) == 0 && ((uintptr_t)Ws & 3) == 0 && ((uintptr_t)qkv & 15) == 0 &&
                ((uintptr_t)q2 & 15) == 0 && ((uintptr_t)k2 & 15) == 0 && ((uintptr_t)cos & 15) == 0 && ((uintptr_t)sin & 15) == 0 &&
                (!bias || ((uintptr_t)bias & 15) == 0) && (!wq || (((uintptr_t)wq | (uintptr_t)wk) & 3) == 0),
                "gemm_nt_qkv_rope_mx8: element operands must start on 128-B lines, scales on 4 B, outputs / tables / bias on 16 B");
  const int M = B * N, Nc = 3 * H * 64;
  EpiArgs e{};
  e.C = qkv; e.ldc = Nc; e.bias = bias; e.rows_per_batch = N; e.f16_max = 65504.f;
  e.q2 = q2; e.k2 = k2; e.wq = wq; e.wk = wk; e.cosT = cos; e.sinT = sin; e.heads = H; e.store_raw_qk = store_raw_qk; e.eps = eps;
  LDMAE_REQUIRE(launch_mx8<bf16>(LDMAE_EPI_QKV_ROPE, Aq, As, Wq, Ws, M, Nc, K, lda, ldb, e, tile_launch, as_stream(stream)),
                "gemm_nt_qkv_rope_mx8: the kernel refused the shape");
  mx8_count(2);
  LDMAE_CHECK_LAUNCH("gemm_nt_qkv_rope_mx8");
  return LDMAE_OK;
}
