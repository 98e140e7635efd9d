// Flash-style attention for the LightningDiT block (hd = 64) on gfx950: softmax(q k^T * scale) v,
// non-causal, no mask (lightningdit.py:76-80).  q,k,v are head-major [B,H,N,hd]; o / do are
// token-major [B,N,H*hd] (the layout the proj GEMM consumes).
//
// bf16 path: mfma_f32_32x32x16_bf16.  Scores are computed TRANSPOSED (S^T = K . Q^T) so a lane owns one
// query column: the row max / row sum are in-register plus one cross-half shuffle, and the f32
// accumulator tile is re-used directly as the B operand of the next product (P^T for O^T = V^T . P^T)
// with the k-order of the 32x32 C/D map (verified by csrc/probe/mfma_probe.hip).  K/V tiles sit in LDS
// in ONE image that serves both row reads (ds_read_b128) and transposed reads (ds_read_b64_tr_b16):
// 8-row x 32-col sub-tiles of 512 B with a 2-bit XOR on the 16-B chunk; filled by global_load_lds with
// the permutation applied to the per-lane SOURCE address.
//
// The loops are bound by vector-instruction ISSUE, not by the matrix pipe (hd = 64: 16 MFMAs against 32 exponentials per 64-key tile
// and wave), so everything around the exponential is folded away: the stationary operand carries scale*log2(e), the score chains start
// from accumulators that already hold -(running max) / -lse / -delta, and tile addresses are scalar (SGPR-base LDS-DMA).
//
// Backward = two passes without atomics (bitwise reproducible):
//   dKdV: a wave owns 32 keys (key on the lane), sweeps 64-query tiles: S, dP, then dV^T += dO^T P,
//         dK^T += Q^T dS with Q / dO read both by rows and transposed from the same LDS image.
//   dQ  : a wave owns 32 queries (query on the lane), sweeps 64-key tiles: S^T, dP^T, dQ^T += K^T dS^T.
// f32 path (parity contract): same structure on mfma_f32_32x32x2f32 with padded f32 LDS tiles.
//
// This header: the device helpers every 16-bit attention kernel uses (the dual-use LDS image, tile staging, register fragments, the
// row-store and fused QK-norm / RoPE backward epilogues).  Included by attention.hip (the product kernels and the C ABI).
#pragma once
#include "common.h"

#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

// byte offset of 16-B chunk `ch` of row `row` in the dual-use LDS image of a [rows][HD] bf16 tile
template <int HD> __device__ __forceinline__ int tile_off(int row, int ch) {
  return (HD * 16) * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}
// inverse: LDS byte offset (multiple of 16) -> (row, ch)
template <int HD> __device__ __forceinline__ void tile_inv(int off, int& row, int& ch) {
  const int grp = off / (HD * 16), within = off % (HD * 16);
  const int sub = within >> 9, rem = within & 511, r7 = rem >> 6, pos = (rem & 63) >> 4;
  row = grp * 8 + r7;
  ch = sub * 4 + (pos ^ ((row >> 2) & 3));
}
// Head dims that are not a multiple of 32 (LightningDiT-XL: 72, VMAE: 16) are tiled with the LDS images and the register
// fragments zero-padded to HDP = the next multiple of 32; global memory keeps the true HD (no padded copies in HBM).  Zero q/k
// columns add 0 to every score, zero v / dO columns produce output columns that are never stored.  Padded 16-B chunks of an
// LDS tile are fetched from this 16 zero bytes (the DMA source address is per lane).
// (`inline`: the three tables are seen by several translation units of one shared library; every code object -- the build has no
// relocatable device code -- keeps its own copy, the host-side shadows merge at the link)
inline __device__ __attribute__((aligned(16))) unsigned g_zero16[4] = {0u, 0u, 0u, 0u};
// 1.0 (bf16) in the first of eight columns: as the first PADDED chunk of a V row it makes column HD of the V image a column of ones, and
// the P.V product then delivers the softmax row sums in accumulator row HD of the (padded) output -- for free, on the matrix pipe
inline __device__ __attribute__((aligned(16))) unsigned g_one16[4] = {0x00003F80u, 0u, 0u, 0u};
inline __device__ __attribute__((aligned(16))) unsigned g_one16h[4] = {0x00003C00u, 0u, 0u, 0u};     // the same column of ones in fp16
constexpr int hd_pad(int hd) { return (hd + 31) / 32 * 32; }

// stage a [ROWS][HD] bf16 tile (global row stride ld elements) into the [ROWS][HDP] LDS image with global_load_lds; 256 threads
template <int HD, int ROWS, bool ONES = false, bool F16 = false>      // ONES: the first padded chunk of every row comes from g_one16 (the forward kernel's V tile)
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ g, long ld, int row_limit, char* lds, int wave, int lane) {
  constexpr int HDP = hd_pad(HD), PIECES = ROWS * HDP * 2 / 1024;
  static_assert(PIECES % 4 == 0 || PIECES == 2 || PIECES == 1, "tile too small");
#pragma unroll
  for (int i = 0; i < (PIECES + 3) / 4; ++i) {
    const int pi = wave * ((PIECES + 3) / 4) + i;
    if (pi < PIECES) {
      int row, ch;
      tile_inv<HDP>(pi * 1024 + lane * 16, row, ch);
      row = min(row, row_limit);
      const void* src = (HD == HDP || ch * 8 < HD) ? (const void*)(g + (long)row * ld + ch * 8)
                                                    : ((ONES && ch * 8 == HD) ? (const void*)(F16 ? g_one16h : g_one16) : (const void*)g_zero16);
      glds16(src, lds + pi * 1024);
    }
  }
}
// The same staging with the addressing hoisted out of the tile loop: per-lane byte offsets of this wave's pieces, computed once; a tile is
// then (uniform base pointer, uniform LDS address) + one LDS-DMA instruction per piece.  Padded head dims (16, 72): the lanes whose chunk
// lies past the true head dim take NO part in the DMA (the instruction runs under an EXEC mask: the hardware writes LDS bytes base + 16 *
// lane for active lanes only), and their sixteen bytes of every LDS image are written ONCE, by `prefill`, before the first tile: zeros, or
// (ONES) the ones column of the forward kernel's V tile.  Round 3 fetched those chunks from 16 zero bytes with a per-lane POINTER, which
// put the whole address computation (~70 vector instructions per tile) back into the tile loop of kernels that are bound by vector issue.
// Every piece has real lanes (checked at compile time for the instantiated head dims), so every wave still issues the same number of
// DMA instructions per tile and the counted vmcnt waits hold.
template <int HD, int ROWS> struct TileMap {
  static constexpr int HDP = hd_pad(HD), PIECES = ROWS * HDP * 2 / 1024, NPW = (PIECES + 3) / 4;
  unsigned voff[NPW];
  unsigned real;                 // bit i: this lane's chunk of piece i lies inside the true head dim
  __device__ __forceinline__ void init(long ld, int wave, int lane) {
    real = 0;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      int row, ch;
      tile_inv<HDP>((wave * NPW + i) * 1024 + lane * 16, row, ch);
      voff[i] = (unsigned)((row * ld + ch * 8) * 2);
      if (ch * 8 < HD) real |= 1u << i;
    }
  }
  // the padded chunks of one LDS tile image (call once per image, then lgkmcnt(0) + a barrier before the first read)
  template <bool ONES = false, bool F16 = false> __device__ __forceinline__ void prefill(char* lds, int wave, int lane) const {
    if constexpr (HD != HDP) {
#pragma unroll
      for (int i = 0; i < NPW; ++i)
        if (wave * NPW + i < PIECES && !((real >> i) & 1u)) {
          int row, ch;
          tile_inv<HDP>((wave * NPW + i) * 1024 + lane * 16, row, ch);
          *(uint4*)(lds + (wave * NPW + i) * 1024 + lane * 16) = make_uint4((ONES && ch * 8 == HD) ? (F16 ? 0x00003C00u : 0x00003F80u) : 0u, 0u, 0u, 0u);
        }
    }
  }
  // g: first element of the tile (wave-uniform); lds_addr: LDS byte address of the tile's image (wave-uniform)
  __device__ __forceinline__ void issue(const bf16* g, long, char*, unsigned lds_addr, int wave, int) const {
#pragma unroll
    for (int i = 0; i < NPW; ++i)
      if (wave * NPW + i < PIECES) {
        if constexpr (HD == HDP) glds16_s(g, voff[i], lds_addr + (wave * NPW + i) * 1024);
        else if ((real >> i) & 1u) glds16_s(g, voff[i], lds_addr + (wave * NPW + i) * 1024);       // EXEC-masked
      }
  }
};
__device__ __forceinline__ unsigned lds_addr_of(const void* p) { return __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_PTR(void, p)); }
// register fragment times a scalar, rounded back to bf16 (the stationary operand of a score product carries scale * log2(e))
__device__ __forceinline__ bf16x8 frag_scale(const bf16x8& a, float c) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)a[j] * c);
  return o;
}
// the fp16 forms (the forward kernel's TF32-class instantiation: fragments keep the bf16x8 REGISTER type, the bits are fp16)
__device__ __forceinline__ bf16x8 frag_scale_h(const bf16x8& a, float c) {
  const f16x8 x = __builtin_bit_cast(f16x8, a);
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = from_f<f16>((float)x[j] * c);
  return __builtin_bit_cast(bf16x8, o);
}
template <bool F16> __device__ __forceinline__ f32x16 mfma_att(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool F16> __device__ __forceinline__ bf16x8 frag_scale_t(const bf16x8& a, float c) {
  if constexpr (F16) return frag_scale_h(a, c); else return frag_scale(a, c);
}
template <bool F16> struct ActT { typedef bf16 t; };
template <> struct ActT<true> { typedef f16 t; };
// dot product of two 8-element register fragments in f32
template <bool F16> __device__ __forceinline__ float frag_dot(const bf16x8& a, const bf16x8& b) {
  float d = 0.f;
  if constexpr (F16) {
    const f16x8 x = __builtin_bit_cast(f16x8, a), y = __builtin_bit_cast(f16x8, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) d += (float)x[j] * (float)y[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) d += (float)a[j] * (float)b[j];
  }
  return d;
}
__device__ __forceinline__ f32x16 splat16(float v) {
  f32x16 o;
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = v;
  return o;
}
// 8 bf16 of a row held in global memory at column c (a register fragment); zero past the true head dim
template <int HD> __device__ __forceinline__ bf16x8 gfrag(const bf16* row, int c) {
  if (HD % 16 == 0 || c < HD) return *(const bf16x8*)(row + c);
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (bf16)0.f;
  return z;
}
// A-operand fragment for a product that contracts over the tile's ROW index (transposed read):
// rows r0 + {4h.. , 8+4h..} in the acc-as-operand k order, 32 columns starting at c0 (lane r = column)
template <int HD> __device__ __forceinline__ bf16x8 frag_tr(const char* tile, int r0, int c0, int lane) {
  const int h = lane >> 5, g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int row = r0 + 4 * h + q, ch = (c0 >> 3) + 2 * (g & 1) + (p >> 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + tile_off<HD>(row, ch) + ((p & 1) << 3)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + tile_off<HD>(row + 8, ch) + ((p & 1) << 3)));
  union { bf16x8 v; s16x4 h2[2]; } u;
  u.h2[0] = lo; u.h2[1] = hi;
  return u.v;
}
// A-operand fragment by rows: row r0 + (lane&31), k chunk (2*ks + h)
template <int HD> __device__ __forceinline__ bf16x8 frag_row(const char* tile, int r0, int ks, int lane) {
  return *(const bf16x8*)(tile + tile_off<HD>(r0 + (lane & 31), 2 * ks + (lane >> 5)));
}
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& x, int s) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (bf16)x[8 * s + j];
  return f;
}
__device__ __forceinline__ bf16x8 acc_frag_h(const f32x16& x, int s) {       // p in [0, 1]: no saturation needed
  f16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (f16)x[8 * s + j];
  return __builtin_bit_cast(bf16x8, f);
}
template <bool F16> __device__ __forceinline__ bf16x8 acc_frag_t(const f32x16& x, int s) {
  if constexpr (F16) return acc_frag_h(x, s); else return acc_frag(x, s);
}
__device__ __forceinline__ int acc_row(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// Sequence lengths that are not a multiple of 64 (VMAE: int(L * (1 - mask_ratio)) kept tokens for any ratio, models_mae.py:472-497): the
// LAST tile of a sweep is ragged.  Its missing rows are staged as copies of row N-1 (finite data, in bounds) and the score-chain
// accumulator rows that belong to them are set to -inf before the exponential: p = exp2(-inf) = 0, so they add nothing to the row sums,
// to O, or to any gradient.  `base` = first row of the 32-row block the accumulator covers; element t of half h is row acc_row(t, h).
__device__ __forceinline__ void mask_rows_past(f32x16& x, int base, int h, int N) {
#pragma unroll
  for (int t = 0; t < 16; ++t)
    if (base + (t & 3) + 8 * (t >> 2) + 4 * h >= N) x[t] = -__builtin_inff();
}

// K/V (Q/dO) tiles travel through a STAGES-deep LDS ring: global_load_lds stays in flight across the per-tile
// barrier (raw s_barrier + counted vmcnt), `ahead` = number of later stages allowed to be still in flight.
template <int PPW, int STAGES> __device__ __forceinline__ void ring_wait(int ahead) {
  if (ahead >= 2) { if constexpr (STAGES >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory"); }
  else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
#define EXP2(x) __builtin_amdgcn_exp2f(x)
constexpr int ATT_STAGES = 3;
// f(IC<0>{}), f(IC<1>{}), ... f(IC<N-1>{}): a loop whose index is a compile-time constant in the body
template <int N, int I = 0, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(IC<I>{}); static_for<N, I + 1>(f); }
}
// running-max update threshold (log2 units): the O / l rescale is skipped while no query of the wave saw its
// maximum grow by more than this (P then stays <= 2^RESCALE_THR; exact softmax either way after the final 1/l)
constexpr float RESCALE_THR = 6.0f;

// ================================================================================================ epilogues
// Epilogue store of a wave's [32 rows][HD] result held as (result)^T accumulators (lane = row r + 32 h; element t of block d is
// column d*32 + 8*(t/4) + 4h + t%4).  Per-lane stores would put 8 B into 32 different rows per instruction (the store tail of a
// workgroup then costs ~9k cycles, MI355X_MICROARCH 'attention epilogue store tail'); instead the tile goes through a wave-private
// LDS image (144-B row pitch) and leaves as whole 128-B rows, 16 B per lane, 8 rows per instruction.  `mul` is per lane (= per row).
template <int HD, typename T = bf16>
__device__ __forceinline__ void store_rows_t(const f32x16 (&acc)[hd_pad(HD) / 32], float mul, char* lds_wave, bf16* gbase, long gstride, int lane,
                                             int nrows = 32) {      // nrows: rows of the wave's 32 that exist (ragged last block when N % 32 != 0)
  constexpr int PITCH = hd_pad(HD) * 2 + 16, CPR = HD / 8;    // bytes per LDS row; 16-B chunks per (true) row
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int d = 0; d < hd_pad(HD) / 32; ++d)
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      typename Pack<T>::v4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = from_f<T>(acc[d][4 * t4 + j] * mul);
      *(typename Pack<T>::v4*)(lds_wave + r * PITCH + (d * 32 + 8 * t4 + 4 * h) * 2) = w;
    }
#pragma unroll
  for (int it = 0; it < (32 * CPR + 63) / 64; ++it) {
    const int idx = it * 64 + lane, row = idx / CPR, ch = idx % CPR;
    if (((32 * CPR) % 64 == 0 || idx < 32 * CPR) && row < nrows) {
      const bf16x8 v = *(const bf16x8*)(lds_wave + row * PITCH + ch * 16);
      *(bf16x8*)(gbase + (long)row * gstride + ch * 8) = v;
    }
  }
}

// ---- QK-RMSNorm + RoPE backward folded into the dQ / dK epilogues (LightningDiT block, head dims with 8 or 16 chunks per row).
// The unfused chain wrote dq / dk head-major, then qk_rope.hip's qknorm_rope_bwd read them back with the pre-norm q / k to produce
// the packed dqkv (1.6 GB per layer at bs 256).  Here the dq (dk) tile goes through the same bf16 row image as store_rows_t and every
// (row, 16-B chunk) lane finishes the job: rope^T, RMSNorm backward against the pre-norm row it loads from the packed qkv, the result
// stored into the q (k) slot of dqkv as a whole 128-B line per row.  Same per-element formulas as qknorm_rope_bwd_kernel.
// Partial sums for the norm-weight and qkv-bias gradients are left per workgroup (batch, 128-row block, head): Pw [B*NB*H][2*hd] (q | k),
// Pb [B*NB][3*H*hd] (q | k | v) with NB = ceil(N / 128), summed over rows by the host (ldmae_colsum).
struct QkNormBwd {
  const bf16* qkv;
  const float* wq; const float* wk; const float* cos; const float* sin;
  bf16* dqkv;
  float* Pw; float* Pb;
  float eps;
};
// sum over the CPR (8 or 16) consecutive lanes that hold one row, by DPP moves (a few cycles each; __shfl_xor is a ds_bpermute round
// trip, and two of these reductions sit in the dependent chain of every row): quad_perm xor 1, xor 2, then row_half_mirror joins the
// two quads of an 8-lane group and row_mirror the two halves of a 16-lane row (the partial sums are uniform inside a group by then)
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CPR> __device__ __forceinline__ float row_sum(float v) {
  v = dpp_add<0xB1>(v);            // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);            // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);           // row_half_mirror
  if constexpr (CPR == 16) v = dpp_add<0x140>(v);      // row_mirror
  return v;
}
template <int CPR> __device__ __forceinline__ float col_sum(float v) {      // over the 64 / CPR lanes that hold one chunk column
#pragma unroll
  for (int o = CPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// everything the epilogue reads from global memory (pre-norm rows: HBM; cos / sin rows: L2-resident tables) is requested BEFORE the
// end-of-loop barrier, all iterations at once, so the latency hides under the barrier and the staging (the main loop's registers are dead)
template <int HD> struct QkPref { bf16x8 x[32 * (HD / 8) / 64]; float4 cs[32 * (HD / 8) / 64][2], sn[32 * (HD / 8) / 64][2]; };
template <int HD>
__device__ __forceinline__ void qk_prefetch_cs(QkPref<HD>& p, const QkNormBwd& a, int n0, int lane) {
  constexpr int CPR = HD / 8;
#pragma unroll
  for (int it = 0; it < 32 * CPR / 64; ++it) {
    const size_t to = (size_t)(n0 + (it * 64 + lane) / CPR) * HD + (lane % CPR) * 8;
    p.cs[it][0] = *(const float4*)(a.cos + to); p.cs[it][1] = *(const float4*)(a.cos + to + 4);
    p.sn[it][0] = *(const float4*)(a.sin + to); p.sn[it][1] = *(const float4*)(a.sin + to + 4);
  }
}
template <int HD>
__device__ __forceinline__ void qk_prefetch(QkPref<HD>& p, const QkNormBwd& a, int which, int b, int hh, int H, int N, int n0, int lane) {
  constexpr int CPR = HD / 8;
#pragma unroll
  for (int it = 0; it < 32 * CPR / 64; ++it) {
    const int row = (it * 64 + lane) / CPR, ch = lane % CPR;
    if (a.wq) p.x[it] = *(const bf16x8*)(a.qkv + (((size_t)b * N + n0 + row) * 3 + which) * H * HD + (size_t)hh * HD + ch * 8);
    else {                                   // RoPE only (use_qknorm=False): the pre-norm rows are not needed; zeros keep the row math finite
#pragma unroll
      for (int j = 0; j < 8; ++j) p.x[it][j] = (bf16)0.f;
    }
  }
}
// The row math of the fused QK-norm / RoPE backward: lane = (row, 16-B chunk) of a wave's 32 rows, `grad(it)` = the lane's 8 incoming
// gradients (already rounded to bf16) of iteration `it`.  aw / ab: this wave's column sums (norm-weight gradient, bias gradient) for
// columns ch*8 .. +7, valid on lanes < CPR
template <int HD, typename GRAD>
__device__ __forceinline__ void qknorm_rows_math(GRAD&& grad, int lane, const QkNormBwd& a, int which, int b, int hh, int H, int N, int n0,
                                                 const QkPref<HD>& pf, float (&aw)[8], float (&ab)[8]) {
  static_assert(HD == 64 || HD == 128, "fused QK-norm backward: 8 or 16 chunks per row");
  constexpr int CPR = HD / 8, NIT = 32 * CPR / 64;
  const int ch = lane % CPR;                      // 64 % CPR == 0: a lane keeps its chunk column in every iteration
  const bool norm = a.wq != nullptr;              // false: q_norm = k_norm = nn.Identity (lightningdit.py:60-61): w = 1, rstd = 1, n = 0 -> the stored row is rope^T(g)
  const float* wsrc = (which ? a.wk : a.wq) + ch * 8;
  float w8[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { w8[j] = norm ? wsrc[j] : 1.f; aw[j] = 0.f; ab[j] = 0.f; }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int row = (it * 64 + lane) / CPR, n = n0 + row;
    const bf16x8 gv = grad(it);
    const size_t so = (((size_t)b * N + n) * 3 + which) * H * HD + (size_t)hh * HD + ch * 8;
    const float c8[8] = {pf.cs[it][0].x, pf.cs[it][0].y, pf.cs[it][0].z, pf.cs[it][0].w, pf.cs[it][1].x, pf.cs[it][1].y, pf.cs[it][1].z, pf.cs[it][1].w};
    const float s8[8] = {pf.sn[it][0].x, pf.sn[it][0].y, pf.sn[it][0].z, pf.sn[it][0].w, pf.sn[it][1].x, pf.sn[it][1].y, pf.sn[it][1].z, pf.sn[it][1].w};
    float x[8], g[8], ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { x[j] = (float)pf.x[it][j]; g[j] = (float)gv[j]; ss += x[j] * x[j]; }
    const float rs = norm ? rsqrtf(row_sum<CPR>(ss) / (float)HD + a.eps) : 1.f;
    float nq[8], dn[8], dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {              // rope^T on the pair (j, j+1): qk_rope.hip rope_apply_bwd
      const float t0 = g[j] * c8[j] + g[j + 1] * s8[j + 1], t1 = g[j + 1] * c8[j + 1] - g[j] * s8[j];
      nq[j] = x[j] * rs; nq[j + 1] = x[j + 1] * rs;
      aw[j] += t0 * nq[j]; aw[j + 1] += t1 * nq[j + 1];
      dn[j] = t0 * w8[j]; dn[j + 1] = t1 * w8[j + 1];
      dot += dn[j] * nq[j] + dn[j + 1] * nq[j + 1];
    }
    const float m = row_sum<CPR>(dot) / (float)HD;
    bf16x8 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) { ov[j] = (bf16)((dn[j] - nq[j] * m) * rs); ab[j] += (float)ov[j]; }
    *(bf16x8*)(a.dqkv + so) = ov;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { aw[j] = col_sum<CPR>(aw[j]); ab[j] = col_sum<CPR>(ab[j]); }
}
// the dq (dk) tile held as (result)^T accumulators: through the wave's bf16 row image (as store_rows_t), then the row math
template <int HD>
__device__ __forceinline__ void qknorm_rows_bwd(const f32x16 (&acc)[HD / 32], float mul, char* lds_wave, int lane, const QkNormBwd& a, int which,
                                                int b, int hh, int H, int N, int n0, const QkPref<HD>& pf, float (&aw)[8], float (&ab)[8]) {
  constexpr int PITCH = HD * 2 + 16, CPR = HD / 8;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int d = 0; d < HD / 32; ++d)
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      bf16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (bf16)(acc[d][4 * t4 + j] * mul);
      *(bf16x4*)(lds_wave + r * PITCH + (d * 32 + 8 * t4 + 4 * h) * 2) = w;
    }
  qknorm_rows_math<HD>([&](int it) { return *(const bf16x8*)(lds_wave + ((it * 64 + lane) / CPR) * PITCH + (lane % CPR) * 16); },
                       lane, a, which, b, hh, H, N, n0, pf, aw, ab);
}
// store_rows_t that also returns the column sums of the rows AS STORED (the v part of the qkv bias gradient): ab, valid on lanes < CPR
template <int HD>
__device__ __forceinline__ void store_rows_t_colsum(const f32x16 (&acc)[HD / 32], float mul, char* lds_wave, bf16* gbase, long gstride, int lane,
                                                    float (&ab)[8]) {
  static_assert(HD == 64 || HD == 128, "8 or 16 chunks per row");
  constexpr int PITCH = HD * 2 + 16, CPR = HD / 8;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int d = 0; d < HD / 32; ++d)
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      bf16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (bf16)(acc[d][4 * t4 + j] * mul);
      *(bf16x4*)(lds_wave + r * PITCH + (d * 32 + 8 * t4 + 4 * h) * 2) = w;
    }
  const int ch = lane % CPR;
#pragma unroll
  for (int j = 0; j < 8; ++j) ab[j] = 0.f;
#pragma unroll
  for (int it = 0; it < 32 * CPR / 64; ++it) {
    const int row = (it * 64 + lane) / CPR;
    const bf16x8 v = *(const bf16x8*)(lds_wave + row * PITCH + ch * 16);
    *(bf16x8*)(gbase + (long)row * gstride + ch * 8) = v;
#pragma unroll
    for (int j = 0; j < 8; ++j) ab[j] += (float)v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) ab[j] = col_sum<CPR>(ab[j]);
}
// the four waves' column sums (NV vectors of HD floats each, lanes < CPR hold 8 columns) -> one row per workgroup, summed in wave order
template <int HD, int NV>
__device__ __forceinline__ void wg_colsums(const float (&v)[NV][8], float* red, int wave, int lane, bool active, int nact, float* const (&dst)[NV]) {
  constexpr int CPR = HD / 8;
  if (active && lane < CPR) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[(wave * NV + k) * HD + lane * 8 + j] = v[k][j];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < NV * HD; t += 256) {
    float s = red[t];
    for (int w = 1; w < nact; ++w) s += red[w * NV * HD + t];
    dst[t / HD][t % HD] = s;
  }
}

// where q / k / v (and dq / dk / dv) live: element offsets of (batch b, head h, row n) = b * sb + h * sh + n * ld.
// Head-major [B,H,N,hd]: sb = H*N*hd, sh = N*hd, ld = hd.  Packed token-major qkv [B,N,3,H,hd] (what the qkv Linear writes, used as is
// by the VMAE blocks, which have no QK-norm / RoPE between the Linear and the attention): sb = N*3*H*hd, sh = hd, ld = 3*H*hd.
struct QkvLayout { long sb, sh, ld; };
static inline QkvLayout layout_hm(int H, int N, int hd) { return {(long)H * N * hd, (long)N * hd, (long)hd}; }
static inline QkvLayout layout_pk(int H, int N, int hd) { return {(long)N * 3 * H * hd, (long)hd, 3L * H * hd}; }

// ================================================================================================ host: launches
// One launch of a kernel with dynamic LDS: the kernel's limit is raised to `lds` on every call (the runtime keeps it per function; no
// state of ours), then the launch.  Every argument is converted to the kernel's own parameter type (the C ABI hands over void*).
template <int THREADS = 256, typename... P, typename... A>
static inline void attn_launch(void (*kernel)(P...), unsigned grid, size_t lds, hipStream_t st, A... args) {
  hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), lds, st, (P)args...);
}
