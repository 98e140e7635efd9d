// Attention for the LightningDiT and VMAE blocks on gfx950: the product kernels (16-bit flash forward, dQ, dK/dV; the f32 parity family)
// and the C ABI.  The scheme (transposed scores, the dual-use LDS image) and the device helpers are in attention_common.h; the concluded
// experiments (one-pass backward, fused head-dim-16 backward) are retired: tools/README.md, "Retired experiments".
#include "attention_common.h"

// ================================================================================================ forward, bf16
// VALU diet (the loop is bound by vector ISSUE, not by the matrix pipe: ~260 VALU instructions per 16 MFMAs before, profiles/r02):
// (i) q carries scale*log2(e) (rounded once more to bf16 in registers) and every score chain starts from the accumulator block
// nm = -(running max): the MFMA result is already the exponent, p = exp2(s) is ONE instruction per score; (ii) the running max only
// moves in the (rare, wave-uniform) rescale branch, which shifts the tile's scores and refreshes nm; (iii) K / V tile addresses are scalar.
// F16: the operands are fp16 (same bytes per element; v_mfma_f32_32x32x16_f16): the TF32-class forward path of the VMAE docking calls
template <int HD, bool RAGGED = false, bool F16 = false>      // RAGGED: N % 64 != 0 (its own instantiation: the masking costs the hot shapes no registers)
__global__ __launch_bounds__(256) void attn_fwd_bf16_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K, const bf16* __restrict__ V,
                                                            bf16* __restrict__ O, float* __restrict__ LSE, int H, int N, float c, QkvLayout L, QkvLayout Lv,
                                                            const float* __restrict__ SB, int sb_heads) {
  constexpr int HDP = hd_pad(HD), KS = (HD + 15) / 16, DB = HDP / 32, TB = 64 * HDP * 2;
  constexpr bool BATCH = HDP <= 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [STAGES][K tile | V tile]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
  const int qblocks = (N + 127) / 128;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lid / qblocks, q0 = (lid % qblocks) * 128 + wave * 32;
  const bool active = q0 < N;
  const size_t hb = (size_t)(bh / H) * L.sb + (size_t)(bh % H) * L.sh;
  const bf16* qp = Q + hb;
  const bf16* kp = K + hb;
  const bf16* vp = V + (size_t)(bh / H) * Lv.sb + (size_t)(bh % H) * Lv.sh;
  const long ld = L.ld, ldv = Lv.ld;
  bf16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16x8 qraw = gfrag<HD>(qp + (size_t)min(q0 + r, N - 1) * ld, ks * 16 + 8 * h);
    qf[ks] = F16 ? frag_scale_h(qraw, c) : frag_scale(qraw, c);
  }
  f32x16 oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) oacc[d] = splat16(0.f);
  f32x16 nm = splat16(0.f);                // -ms in every element: the C operand of the first MFMA of a score chain
  float ms = 0.f, l = 0.f;                 // ms is set from the first tile (rescale branch), so 0 is never used as a maximum
  const int nt = (N + 63) / 64;
  constexpr bool ragged = RAGGED;          // the last key tile has N % 64 real rows (see mask_rows_past)
  constexpr int PPW = 2 * (TB / 1024) / 4;
  TileMap<HD, 64> mk, mv;
  mk.init(ld, wave, lane);
  mv.init(ldv, wave, lane);
  // padded head dims: the row sums come out of the P.V product (ones column in the V image, see g_one16) instead of 32 vector adds per tile
  constexpr bool LSUM = HD != HDP;
  constexpr int LROW = HD % 32, LREG = (LROW & 3) + 4 * (LROW >> 3), LHALF = (LROW >> 2) & 1;
  if constexpr (HD != HDP) {
#pragma unroll
    for (int st = 0; st < ATT_STAGES; ++st) {
      mk.prefill(smem + st * 2 * TB, wave, lane);
      mv.template prefill<true, F16>(smem + st * 2 * TB + TB, wave, lane);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0): in LDS before this wave reaches the first tile barrier
  }
  // A STATIC shift instead of the running maximum, when the caller can bound the scores (SB: one float on the device, an upper bound of
  // |score * scale * log2(e)| over all queries and keys -- for the QK-normalised DiT heads it follows from the norm weights alone:
  // ldmae_qk_score_bound).  With the shift bq every exponent s - bq lies in [-2 bq, 0]: no p overflows, and while 2 bq <= 100 none flushes
  // to zero, so the softmax is exact without the per-tile 31-deep max chain, cross-half shuffle, ballot and rescale branch (a fifth of the
  // loop's vector instructions: -8 % at head dim 64, -12 % at 16, profiles/r04_attn_static_shift.txt).  No bound, or one above 50: the
  // tracked form below, as before.
  // sb_heads: SB is [B*H][2] = (max_i |q_i|^2, max_j |k_j|^2) of each (batch, head) as STORED (unscaled): |q_i . k_j| <= |q_i| |k_j|
  // (the fused VMAE q | k | v kernel leaves these maxima behind for free: csrc/vmae_fused.hip).
  // A first value of 0 means "no maximum over the queries": every lane then uses the norm of its own (scaled) query (ldmae_k_norm_max).
  float bq = 0.f;
  if (SB && !F16) {                         // (the fp16 instantiation keeps the tracked form: its callers pass no bound)
    if (!sb_heads) bq = *SB;
    else if (SB[2 * bh] > 0.f) bq = sqrtf(SB[2 * bh] * SB[2 * bh + 1]) * c * 1.02f;
    else {
      float qn = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) qn += (float)qf[ks][j] * (float)qf[ks][j];
      qn += __shfl_xor(qn, 32, 64);
      bq = sqrtf(qn * SB[2 * bh + 1]) * 1.02f + 0.01f;
    }
  }
  const bool stat = SB != nullptr && !F16 && __builtin_amdgcn_ballot_w64(!(bq <= 50.f)) == 0;       // wave-uniform
  const unsigned lds0 = lds_addr_of(smem);
  auto stage = [&](int kt) {
    const int so = (kt % ATT_STAGES) * 2 * TB;
    if (ragged && kt == nt - 1) {          // same number of LDS-DMA instructions per wave as the hoisted form: the vmcnt counts hold
      stage_tile<HD, 64>(kp + (size_t)kt * 64 * ld, ld, N - 1 - kt * 64, smem + so, wave, lane);
      stage_tile<HD, 64, LSUM, F16>(vp + (size_t)kt * 64 * ldv, ldv, N - 1 - kt * 64, smem + so + TB, wave, lane);
      return;
    }
    mk.issue(kp + (size_t)kt * 64 * ld, ld, smem + so, lds0 + so, wave, lane);
    mv.issue(vp + (size_t)kt * 64 * ldv, ldv, smem + so + TB, lds0 + so + TB, wave, lane);
  };
#pragma unroll
  for (int st = 0; st < ATT_STAGES - 1; ++st)
    if (st < nt) stage(st);
  // vmcnt(0) through the BUILTIN (visible to the compiler's waitcnt pass): the register fragments above are then known to have
  // landed, so no compiler-counted wait for them ends up inside the tile loop, where -- the ring DMA being hidden in asm -- it
  // would drain the ring at every tile.  The prologue stages are in flight beside those loads, so this costs one round trip.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  auto body = [&](auto ST, auto TRK, int kt) {
    constexpr int st = decltype(ST)::value;
    constexpr bool track = decltype(TRK)::value != 0;
    ring_wait<PPW, ATT_STAGES>(min(ATT_STAGES - 2, nt - 1 - kt));
    __builtin_amdgcn_s_barrier();
    if (kt + ATT_STAGES - 1 < nt) stage(kt + ATT_STAGES - 1);
    const char* Kt = smem + st * 2 * TB;
    const char* Vt = Kt + TB;
    // LDS reads are batched ahead of the MFMAs that consume them (left to itself the compiler keeps ONE fragment in flight and waits
    // for it before every MFMA: 16 exposed LDS round trips per tile); the two 32-key chains are interleaved
    // (head dims up to 64; wider ones would not fit the register file that way and read each fragment where it is used)
    f32x16 s[2];
    bf16x8 kfr[KS][2];
    if constexpr (BATCH) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) kfr[ks][kb] = frag_row<HDP>(Kt, kb * 32, ks, lane);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        s[kb] = mfma_att<F16>(BATCH ? kfr[ks][kb] : frag_row<HDP>(Kt, kb * 32, ks, lane), qf[ks], ks == 0 ? nm : s[kb]);
    bf16x8 vfr[2][2][DB];                              // V^T fragments: in flight under the softmax arithmetic
    if constexpr (BATCH) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int d = 0; d < DB; ++d) vfr[kb][s2][d] = frag_tr<HDP>(Vt, kb * 32 + 16 * s2, d * 32, lane);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ragged && kt == nt - 1) { mask_rows_past(s[0], kt * 64, h, N); mask_rows_past(s[1], kt * 64 + 32, h, N); }
    // s = score * scale * log2(e) - ms
    if constexpr (track) {
      float mx = fmaxf(s[0][0], s[1][0]);
  #pragma unroll
      for (int t = 1; t < 16; ++t) mx = fmaxf(mx, fmaxf(s[0][t], s[1][t]));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const bool first = kt == 0;
      if (first || __builtin_amdgcn_ballot_w64(mx > RESCALE_THR) != 0) {      // wave-uniform: first tile, or some query's max grew a lot
        const float d = first ? mx : fmaxf(mx, 0.f);
        ms += d;
        if (!first) {
          const float alpha = EXP2(-d);
          l *= alpha;
  #pragma unroll
          for (int dd = 0; dd < DB; ++dd)
  #pragma unroll
            for (int t = 0; t < 16; ++t) oacc[dd][t] *= alpha;
        }
  #pragma unroll
        for (int t = 0; t < 16; ++t) { s[0][t] -= d; s[1][t] -= d; }
        nm = splat16(-ms);
      }
    }
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 16; ++t) { const float p = EXP2(s[kb][t]); s[kb][t] = p; if constexpr (!LSUM) rs += p; }
    l += rs;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = F16 ? acc_frag_h(s[kb], s2) : acc_frag(s[kb], s2);
#pragma unroll
        for (int d = 0; d < DB; ++d)
          oacc[d] = mfma_att<F16>(BATCH ? vfr[kb][s2][d] : frag_tr<HDP>(Vt, kb * 32 + 16 * s2, d * 32, lane), pf, oacc[d]);
      }
  };
  if (stat) {                               // the shift is the bound: no maximum to track
    ms = bq;
    nm = splat16(-bq);
    for (int kt = 0; kt < nt; kt += ATT_STAGES) {
      body(IC<0>{}, IC<0>{}, kt);
      if (kt + 1 < nt) body(IC<1>{}, IC<0>{}, kt + 1);
      if (kt + 2 < nt) body(IC<2>{}, IC<0>{}, kt + 2);
    }
  } else {
    for (int kt = 0; kt < nt; kt += ATT_STAGES) {
      body(IC<0>{}, IC<1>{}, kt);
      if (kt + 1 < nt) body(IC<1>{}, IC<1>{}, kt + 1);
      if (kt + 2 < nt) body(IC<2>{}, IC<1>{}, kt + 2);
    }
  }
  if constexpr (LSUM) l = __shfl(oacc[HD / 32][LREG], (lane & 31) + 32 * LHALF, 64);      // row HD of O^T = sum over the keys of P (as rounded to bf16)
  else l += __shfl_xor(l, 32, 64);
  __syncthreads();                                   // every wave is past its last K/V read: the ring becomes store scratch
  if (!active) return;
  const float inv = 1.f / l;
  const int b = bh / H, hh = bh % H;
  if constexpr (F16) store_rows_t<HD, f16>(oacc, inv, smem + wave * 32 * (HDP * 2 + 16), O + ((size_t)(b * N + q0) * H + hh) * HD, (long)H * HD, lane, N - q0);
  else store_rows_t<HD>(oacc, inv, smem + wave * 32 * (HDP * 2 + 16), O + ((size_t)(b * N + q0) * H + hh) * HD, (long)H * HD, lane, N - q0);
  if (h == 0 && q0 + r < N) LSE[(size_t)bh * N + q0 + r] = (ms + log2f(l)) * 0.6931471805599453f;
}

// delta[b,h,n] = sum_d o[b,n,h,d] * do[b,n,h,d]
template <typename T>
__global__ void attn_delta_kernel(const T* __restrict__ O, const T* __restrict__ dO, float* __restrict__ delta, int B, int H, int N, int hd) {
  const long items = (long)B * N * H;
  const int lpr = 8;                     // lanes per (b,n,h) row
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / lpr;
  const int sub = threadIdx.x % lpr;
  for (long it = gid; it < items; it += (long)gridDim.x * 256 / lpr) {
    const int hh = it % H, n = (it / H) % N, b = it / ((long)H * N);
    const T* o = O + (size_t)it * hd;
    const T* g = dO + (size_t)it * hd;
    float s = 0.f;
    for (int d = sub * 8; d < hd; d += lpr * 8) {
      float a[8], e[8];
      Vec8<T>::load(o + d, a); Vec8<T>::load(g + d, e);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += a[j] * e[j];
    }
    s = group_sum<8>(s);
    if (sub == 0) delta[((size_t)b * H + hh) * N + n] = s;
  }
}

// ================================================================================================ backward dK/dV, bf16
// ROWC = [2][B*H*N] f32 written by the dQ kernel (which runs first): slot 0 = -delta, slot 1 = -lse * log2(e).  They are the INITIAL
// ACCUMULATORS of the dP and S chains (a query row = an accumulator element here, so they come from the LDS copy of the tile's 64 values
// by ds_read_b128), k carries scale*log2(e): p = exp2(S) and dS = p * dP are one instruction per element each.
// PF (round 6): LDS operand fragments are requested PF MFMAs ahead of the one that consumes them (a ring of PF + 1 fragments in registers, the
// reads pinned in place against the scheduler), instead of right in front of it behind an `s_waitcnt lgkmcnt(0)` each
template <int HD, bool QKN = false, bool RAGGED = false, bool F16 = false, int PF = 0>      // F16: fp16 operands / outputs (VMAE pre-training under fp16 autocast), QKN = false only
__global__ __launch_bounds__(256) void attn_bwd_dkdv_bf16_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K, const bf16* __restrict__ V,
                                                                 const bf16* __restrict__ dO, const float* __restrict__ ROWC, long rc_stride,
                                                                 bf16* __restrict__ dK, bf16* __restrict__ dV,
                                                                 int H, int N, float scale, QkvLayout L, QkvLayout Lv, QkNormBwd qn) {
  constexpr int HDP = hd_pad(HD), KS = (HD + 15) / 16, DB = HDP / 32, TB = 64 * HDP * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [STAGES][Q tile | dO tile | -lse2[64] -delta[64] scratch[128]]
  constexpr int BUF = 2 * TB + 1024;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
  const float c = scale * 1.4426950408889634f;
  const int kblocks = (N + 127) / 128;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lid / kblocks, k0 = (lid % kblocks) * 128 + wave * 32;
  const bool active = k0 < N;
  const int b = bh / H, hh = bh % H;
  const size_t hb = (size_t)b * L.sb + (size_t)hh * L.sh, hbv = (size_t)b * Lv.sb + (size_t)hh * Lv.sh;
  const long ld = L.ld;
  const bf16* qp = Q + hb;
  const bf16* dop = dO + ((size_t)b * N * H + hh) * HD;     // row stride H*HD
  const long dold = (long)H * HD;
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = frag_scale_t<F16>(gfrag<HD>(K + hb + (size_t)min(k0 + r, N - 1) * ld, ks * 16 + 8 * h), c);
    vf[ks] = gfrag<HD>(V + hbv + (size_t)min(k0 + r, N - 1) * Lv.ld, ks * 16 + 8 * h);
  }
  f32x16 dkacc[DB], dvacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) { dkacc[d] = splat16(0.f); dvacc[d] = splat16(0.f); }
  const int nt = (N + 63) / 64, NP = nt * 64;      // ROWC rows are padded to whole tiles: the dQ kernel fills the pad with (-inf, 0)
  constexpr bool ragged = RAGGED;
  constexpr int PPW = 2 * (TB / 1024) / 4 + 1;
  const float* rowc = ROWC + (size_t)bh * NP + ((wave & 1) ? 0 : rc_stride);     // wave 0/2: -lse2, wave 1/3: -delta
  TileMap<HD, 64> mq, mo;
  mq.init(ld, wave, lane);
  mo.init(dold, wave, lane);
  if constexpr (HD != HDP) {                   // zero padding of every Q / dO image, once (TileMap)
#pragma unroll
    for (int st = 0; st < ATT_STAGES; ++st) { mq.prefill(smem + st * BUF, wave, lane); mo.prefill(smem + st * BUF + TB, wave, lane); }
    __builtin_amdgcn_s_waitcnt(0xC07F);
  }
  const unsigned lds0 = lds_addr_of(smem);
  auto stage = [&](int qt) {
    const int so = (qt % ATT_STAGES) * BUF;
    if (ragged && qt == nt - 1) {          // missing query rows: copies of row N-1; their -lse2 = -inf in ROWC zeroes p (and with it dS)
      stage_tile<HD, 64>(qp + (size_t)qt * 64 * ld, ld, N - 1 - qt * 64, smem + so, wave, lane);
      stage_tile<HD, 64>(dop + (size_t)qt * 64 * dold, dold, N - 1 - qt * 64, smem + so + TB, wave, lane);
    } else {
    mq.issue(qp + (size_t)qt * 64 * ld, ld, smem + so, lds0 + so, wave, lane);
    mo.issue(dop + (size_t)qt * 64 * dold, dold, smem + so + TB, lds0 + so + TB, wave, lane);
    }
    // 64 floats of -lse2 (slot 0) / -delta (slot 1); waves 2,3 fill scratch slots so every wave issues PPW loads
    glds4_s(rowc + qt * 64, lane * 4, lds0 + so + 2 * TB + wave * 256);
  };
#pragma unroll
  for (int st = 0; st < ATT_STAGES - 1; ++st)
    if (st < nt) stage(st);
  // vmcnt(0) through the BUILTIN (visible to the compiler's waitcnt pass): the register fragments above are then known to have
  // landed, so no compiler-counted wait for them ends up inside the tile loop, where -- the ring DMA being hidden in asm -- it
  // would drain the ring at every tile.  The prologue stages are in flight beside those loads, so this costs one round trip.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  auto body = [&](auto ST, int qt) {
    constexpr int st = decltype(ST)::value;
    ring_wait<PPW, ATT_STAGES>(min(ATT_STAGES - 2, nt - 1 - qt));
    __builtin_amdgcn_s_barrier();
    if (qt + ATT_STAGES - 1 < nt) stage(qt + ATT_STAGES - 1);
    const char* Qt = smem + st * BUF;
    const char* dOt = Qt + TB;
    const float* nl = (const float*)(Qt + 2 * TB);
    const float* nd = nl + 64;
    if constexpr (PF > 0) {
      // the 2 x (2 KS + 4 DB) MFMAs of the tile in their order, each with ONE operand fragment from LDS: fragment i + PF is requested before MFMA i
      constexpr int N1 = 2 * KS, N2 = 4 * DB, NQ = N1 + N2, NF = 2 * NQ;
      // sequence position i -> (half qb, step j of that half's N1 + N2 MFMAs)
      auto frag = [&](auto I) -> bf16x8 {
        constexpr int i = decltype(I)::value, qb = i / NQ, j = i % NQ;
        if constexpr (j < N1) {
          if constexpr ((j & 1) != 0) return frag_row<HDP>(dOt, qb * 32, j / 2, lane); else return frag_row<HDP>(Qt, qb * 32, j / 2, lane);
        } else {
          constexpr int t = j - N1, s2 = t / (2 * DB), d = (t % (2 * DB)) / 2;
          if constexpr ((t & 1) != 0) return frag_tr<HDP>(Qt, qb * 32 + 16 * s2, d * 32, lane); else return frag_tr<HDP>(dOt, qb * 32 + 16 * s2, d * 32, lane);
        }
      };
      bf16x8 win[PF + 1];
      static_for<PF>([&](auto I) { win[decltype(I)::value] = frag(I); });
      f32x16 s, dp;
      bf16x8 pf, dsf;
      static_for<NF>([&](auto I) {
        constexpr int i = decltype(I)::value, qb = i / NQ, j = i % NQ;
        if constexpr (i + PF < NF) win[(i + PF) % (PF + 1)] = frag(IC<i + PF>{});
        if constexpr (j == 0) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 a = *(const f32x4*)(nl + qb * 32 + 8 * g + 4 * h), e = *(const f32x4*)(nd + qb * 32 + 8 * g + 4 * h);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) { s[4 * g + jj] = a[jj]; dp[4 * g + jj] = e[jj]; }
          }
        }
        __builtin_amdgcn_sched_barrier(0x6);          // vector / scalar ALU may move across; LDS reads and MFMAs keep this order
        // the exponentials of a half: written where its score chains end
        if constexpr (j == N1) {
#pragma unroll
          for (int t = 0; t < 16; ++t) { const float p = EXP2(s[t]); s[t] = p; dp[t] *= p; }
        }
        if constexpr (j >= N1 && (j - N1) % (2 * DB) == 0) { pf = acc_frag_t<F16>(s, (j - N1) / (2 * DB)); dsf = acc_frag_t<F16>(dp, (j - N1) / (2 * DB)); }
        const bf16x8 a = win[i % (PF + 1)];
        if constexpr (j < N1) {
          if constexpr ((j & 1) != 0) dp = mfma_att<F16>(a, vf[j / 2], dp); else s = mfma_att<F16>(a, kf[j / 2], s);
        } else {
          constexpr int d = ((j - N1) % (2 * DB)) / 2;
          if constexpr (((j - N1) & 1) != 0) dkacc[d] = mfma_att<F16>(a, dsf, dkacc[d]); else dvacc[d] = mfma_att<F16>(a, pf, dvacc[d]);
        }
      });
    } else
    // (fragments are read where they are used: batching them ALL ahead, as the forward kernel does, costs this kernel its third wave per SIMD
    // and measured slower: 1.64 vs 1.56 ms)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16 s, dp;
#pragma unroll
      for (int g = 0; g < 4; ++g) {              // accumulator element 4g+j <-> query row qb*32 + 8g + 4h + j
        const f32x4 a = *(const f32x4*)(nl + qb * 32 + 8 * g + 4 * h), e = *(const f32x4*)(nd + qb * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[4 * g + j] = a[j]; dp[4 * g + j] = e[j]; }
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s = mfma_att<F16>(frag_row<HDP>(Qt, qb * 32, ks, lane), kf[ks], s);
        dp = mfma_att<F16>(frag_row<HDP>(dOt, qb * 32, ks, lane), vf[ks], dp);
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float p = EXP2(s[t]);
        s[t] = p;
        dp[t] *= p;
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = acc_frag_t<F16>(s, s2), dsf = acc_frag_t<F16>(dp, s2);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          dvacc[d] = mfma_att<F16>(frag_tr<HDP>(dOt, qb * 32 + 16 * s2, d * 32, lane), pf, dvacc[d]);
          dkacc[d] = mfma_att<F16>(frag_tr<HDP>(Qt, qb * 32 + 16 * s2, d * 32, lane), dsf, dkacc[d]);
        }
      }
    }
  };
  for (int qt = 0; qt < nt; qt += ATT_STAGES) {
    body(IC<0>{}, qt);
    if (qt + 1 < nt) body(IC<1>{}, qt + 1);
    if (qt + 2 < nt) body(IC<2>{}, qt + 2);
  }
  if constexpr (QKN) {       // dk -> k slot of dqkv through the QK-norm / RoPE backward; dv as before, plus its column sums for the qkv bias gradient
    QkPref<HD> pf;
    if (active) qk_prefetch<HD>(pf, qn, 1, b, hh, H, N, k0, lane);
    __syncthreads();                                 // ring -> store scratch
    char* sw = smem + wave * 32 * (HDP * 2 + 16);
    float cs3[3][8];
    if (active) {
      qk_prefetch_cs<HD>(pf, qn, k0, lane);          // (two accumulator sets are still live before the barrier: no room there)
      qknorm_rows_bwd<HD>(dkacc, scale, sw, lane, qn, 1, b, hh, H, N, k0, pf, cs3[0], cs3[1]);
      store_rows_t_colsum<HD>(dvacc, 1.f, sw, dV + hbv + (size_t)k0 * Lv.ld, Lv.ld, lane, cs3[2]);
    }
    const int kb = lid % kblocks;
    const size_t blk = (size_t)b * kblocks + kb;
    float* const dst[3] = {qn.Pw + (blk * H + hh) * (2 * HD) + HD, qn.Pb + blk * (3 * H * HD) + ((size_t)H + hh) * HD,
                           qn.Pb + blk * (3 * H * HD) + ((size_t)2 * H + hh) * HD};
    wg_colsums<HD, 3>(cs3, (float*)(smem + 4 * 32 * (HDP * 2 + 16)), wave, lane, active, min(4, (N - kb * 128) / 32), dst);
  } else {
    __syncthreads();                                   // ring -> store scratch
    if (!active) return;
    char* sw = smem + wave * 32 * (HDP * 2 + 16);
    store_rows_t<HD, typename ActT<F16>::t>(dkacc, scale, sw, dK + hb + (size_t)k0 * ld, ld, lane, N - k0);
    store_rows_t<HD, typename ActT<F16>::t>(dvacc, 1.f, sw, dV + hbv + (size_t)k0 * Lv.ld, Lv.ld, lane, N - k0);       // same wave, same scratch: LDS ops stay in order
  }
}

// ================================================================================================ backward dQ, bf16
template <int HD, bool QKN = false, bool RAGGED = false, bool F16 = false, int PF = 0>      // F16: fp16 operands / outputs (VMAE pre-training under fp16 autocast), QKN = false only; PF: see the dK/dV kernel
__global__ __launch_bounds__(256) void attn_bwd_dq_bf16_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K, const bf16* __restrict__ V,
                                                               const bf16* __restrict__ O, const bf16* __restrict__ dO,
                                                               const float* __restrict__ LSE, float* __restrict__ ROWC, long rc_stride,
                                                               bf16* __restrict__ dQ, int H, int N, float scale, QkvLayout L, QkvLayout Lv, QkNormBwd qn) {
  constexpr int HDP = hd_pad(HD), KS = (HD + 15) / 16, DB = HDP / 32, TB = 64 * HDP * 2;
  constexpr bool BTR = HDP <= 64;     // transposed K fragments read ahead, under the exp / multiply arithmetic (fits 3 waves per SIMD)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [STAGES][K tile | V tile]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
  const float c = scale * 1.4426950408889634f;
  const int qblocks = (N + 127) / 128;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lid / qblocks, q0 = (lid % qblocks) * 128 + wave * 32;
  const bool active = q0 < N;
  const int b = bh / H, hh = bh % H;
  const int qrow = min(q0 + r, N - 1);
  const size_t hb = (size_t)b * L.sb + (size_t)hh * L.sh;
  const long ld = L.ld, ldv = Lv.ld;
  const bf16* kp = K + hb;
  const bf16* vp = V + (size_t)b * Lv.sb + (size_t)hh * Lv.sh;
  bf16x8 qf[KS], dof[KS];
  // delta_i = sum_d dO[i,d] * O[i,d] is formed here from the dO fragments this lane holds anyway (its half of the row; the other
  // half sits on lane ^ 32) and published (negated, with -lse*log2(e) beside it) for the dK/dV kernel, which runs after this one:
  // no separate pass over O and dO.  Here the query sits on the lane, so both are lane constants: splat into the accumulator blocks
  // the S and dP chains start from; q carries scale*log2(e).
  float dpart = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = frag_scale_t<F16>(gfrag<HD>(Q + hb + (size_t)qrow * ld, ks * 16 + 8 * h), c);
    const size_t oo = (((size_t)b * N + qrow) * H + hh) * HD;
    dof[ks] = gfrag<HD>(dO + oo, ks * 16 + 8 * h);
    const bf16x8 of = gfrag<HD>(O + oo, ks * 16 + 8 * h);
    dpart += frag_dot<F16>(dof[ks], of);
  }
  const float dl = dpart + __shfl_xor(dpart, 32);
  const float lse2 = LSE[(size_t)bh * N + qrow] * 1.4426950408889634f;
  const int NP = (N + 63) / 64 * 64;        // ROWC rows padded to whole tiles; pad rows (-delta, -lse2) = (0, -inf): p = dS = 0 in the dK/dV kernel
  if (h == 0 && q0 + r < NP) {
    const bool real = q0 + r < N;
    ROWC[(size_t)bh * NP + q0 + r] = real ? -dl : 0.f;
    ROWC[rc_stride + (size_t)bh * NP + q0 + r] = real ? -lse2 : -__builtin_inff();
  }
  const f32x16 nl = splat16(-lse2), nd = splat16(-dl);
  f32x16 dqacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) dqacc[d] = splat16(0.f);
  const int nt = (N + 63) / 64;
  constexpr bool ragged = RAGGED;
  constexpr int PPW = 2 * (TB / 1024) / 4;
  TileMap<HD, 64> mk, mv;
  mk.init(ld, wave, lane);
  mv.init(ldv, wave, lane);
  if constexpr (HD != HDP) {                   // zero padding of every K / V image, once (TileMap)
#pragma unroll
    for (int st = 0; st < ATT_STAGES; ++st) { mk.prefill(smem + st * 2 * TB, wave, lane); mv.prefill(smem + st * 2 * TB + TB, wave, lane); }
    __builtin_amdgcn_s_waitcnt(0xC07F);
  }
  const unsigned lds0 = lds_addr_of(smem);
  auto stage = [&](int kt) {
    const int so = (kt % ATT_STAGES) * 2 * TB;
    if (ragged && kt == nt - 1) {
      stage_tile<HD, 64>(kp + (size_t)kt * 64 * ld, ld, N - 1 - kt * 64, smem + so, wave, lane);
      stage_tile<HD, 64>(vp + (size_t)kt * 64 * ldv, ldv, N - 1 - kt * 64, smem + so + TB, wave, lane);
      return;
    }
    mk.issue(kp + (size_t)kt * 64 * ld, ld, smem + so, lds0 + so, wave, lane);
    mv.issue(vp + (size_t)kt * 64 * ldv, ldv, smem + so + TB, lds0 + so + TB, wave, lane);
  };
#pragma unroll
  for (int st = 0; st < ATT_STAGES - 1; ++st)
    if (st < nt) stage(st);
  // vmcnt(0) through the BUILTIN (visible to the compiler's waitcnt pass): the register fragments above are then known to have
  // landed, so no compiler-counted wait for them ends up inside the tile loop, where -- the ring DMA being hidden in asm -- it
  // would drain the ring at every tile.  The prologue stages are in flight beside those loads, so this costs one round trip.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  auto body = [&](auto ST, int kt) {
    constexpr int st = decltype(ST)::value;
    ring_wait<PPW, ATT_STAGES>(min(ATT_STAGES - 2, nt - 1 - kt));
    __builtin_amdgcn_s_barrier();
    if (kt + ATT_STAGES - 1 < nt) stage(kt + ATT_STAGES - 1);
    const char* Kt = smem + st * 2 * TB;
    const char* Vt = Kt + TB;
    if constexpr (PF > 0) {
      // the 2 x (2 KS + 2 DB) MFMAs of the tile in their order, each with ONE operand fragment from LDS (K / V rows for the score chains, transposed
      // K for dQ): fragment i + PF is requested before MFMA i; replaces the batch of transposed reads (BTR) of the PF = 0 form
      constexpr int N1 = 2 * KS, N2 = 2 * DB, NQ = N1 + N2, NF = 2 * NQ;
      auto frag = [&](auto I) -> bf16x8 {
        constexpr int i = decltype(I)::value, kb = i / NQ, j = i % NQ;
        if constexpr (j < N1) {
          if constexpr ((j & 1) != 0) return frag_row<HDP>(Vt, kb * 32, j / 2, lane); else return frag_row<HDP>(Kt, kb * 32, j / 2, lane);
        } else return frag_tr<HDP>(Kt, kb * 32 + 16 * ((j - N1) / DB), ((j - N1) % DB) * 32, lane);
      };
      bf16x8 win[PF + 1];
      static_for<PF>([&](auto I) { win[decltype(I)::value] = frag(I); });
      f32x16 s, dp;
      bf16x8 dsf;
      static_for<NF>([&](auto I) {
        constexpr int i = decltype(I)::value, kb = i / NQ, j = i % NQ;
        if constexpr (i + PF < NF) win[(i + PF) % (PF + 1)] = frag(IC<i + PF>{});
        __builtin_amdgcn_sched_barrier(0x6);          // vector / scalar ALU may move across; LDS reads and MFMAs keep this order
        if constexpr (j == N1) {
          if (ragged && kt == nt - 1) mask_rows_past(s, kt * 64 + kb * 32, h, N);
#pragma unroll
          for (int t = 0; t < 16; ++t) dp[t] *= EXP2(s[t]);
        }
        if constexpr (j >= N1 && (j - N1) % DB == 0) dsf = acc_frag_t<F16>(dp, (j - N1) / DB);
        const bf16x8 a = win[i % (PF + 1)];
        if constexpr (j < N1) {
          if constexpr ((j & 1) != 0) dp = mfma_att<F16>(a, dof[j / 2], j == 1 ? nd : dp); else s = mfma_att<F16>(a, qf[j / 2], j == 0 ? nl : s);
        } else dqacc[(j - N1) % DB] = mfma_att<F16>(a, dsf, dqacc[(j - N1) % DB]);
      });
    } else
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 s, dp;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s = mfma_att<F16>(frag_row<HDP>(Kt, kb * 32, ks, lane), qf[ks], ks == 0 ? nl : s);
        dp = mfma_att<F16>(frag_row<HDP>(Vt, kb * 32, ks, lane), dof[ks], ks == 0 ? nd : dp);
      }
      if (ragged && kt == nt - 1) mask_rows_past(s, kt * 64 + kb * 32, h, N);       // keys past N: p = 0, dS = 0
      bf16x8 ktr[2][DB];
      if constexpr (BTR) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int d = 0; d < DB; ++d) ktr[s2][d] = frag_tr<HDP>(Kt, kb * 32 + 16 * s2, d * 32, lane);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) dp[t] *= EXP2(s[t]);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 dsf = acc_frag_t<F16>(dp, s2);
#pragma unroll
        for (int d = 0; d < DB; ++d) dqacc[d] = mfma_att<F16>(BTR ? ktr[s2][d] : frag_tr<HDP>(Kt, kb * 32 + 16 * s2, d * 32, lane), dsf, dqacc[d]);
      }
    }
  };
  for (int kt = 0; kt < nt; kt += ATT_STAGES) {
    body(IC<0>{}, kt);
    if (kt + 1 < nt) body(IC<1>{}, kt + 1);
    if (kt + 2 < nt) body(IC<2>{}, kt + 2);
  }
  if constexpr (QKN) {
    QkPref<HD> pf;
    if (active) { qk_prefetch<HD>(pf, qn, 0, b, hh, H, N, q0, lane); qk_prefetch_cs<HD>(pf, qn, q0, lane); }
    __syncthreads();                                 // ring -> store scratch
    float cs2[2][8];
    if (active) qknorm_rows_bwd<HD>(dqacc, scale, smem + wave * 32 * (HDP * 2 + 16), lane, qn, 0, b, hh, H, N, q0, pf, cs2[0], cs2[1]);
    const int qb = lid % qblocks;
    const size_t blk = (size_t)b * qblocks + qb;
    float* const dst[2] = {qn.Pw + (blk * H + hh) * (2 * HD), qn.Pb + blk * (3 * H * HD) + (size_t)hh * HD};
    wg_colsums<HD, 2>(cs2, (float*)(smem + 4 * 32 * (HDP * 2 + 16)), wave, lane, active, min(4, (N - qb * 128) / 32), dst);
  } else {
    __syncthreads();                                   // ring -> store scratch
    if (!active) return;
    store_rows_t<HD, typename ActT<F16>::t>(dqacc, scale, smem + wave * 32 * (HDP * 2 + 16), dQ + hb + (size_t)q0 * ld, ld, lane, N - q0);
  }
}

// ================================================================================================ f32 path (parity)
// Tiles are f32 [rows][LD] with LD = HD + 1 (odd stride: conflict-free row reads); operands are single
// floats: A[i = lane&31][k = lane>>5], B[k = lane>>5][j = lane&31] per 32x32x2 step.
template <int HD, int ROWS>
__device__ __forceinline__ void stage_tile_f32(const float* __restrict__ g, long ld, int nrows_valid, float* lds) {
  constexpr int LD = HD + 1;
  for (int i = threadIdx.x; i < ROWS * HD; i += 256) {
    const int row = i / HD, d = i % HD;
    lds[row * LD + d] = row < nrows_valid ? g[(long)row * ld + d] : 0.f;
  }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                           float* __restrict__ O, float* __restrict__ LSE, int H, int N, float c) {
  constexpr int LD = HD + 1, DB = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = (float*)smem;            // [128][LD]
  float* Ks = Qs + 128 * LD;           // [64][LD]
  float* Vs = Ks + 64 * LD;            // [64][LD]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int qblocks = (N + 127) / 128;
  const int bh = blockIdx.x / qblocks, qb0 = (blockIdx.x % qblocks) * 128, q0 = qb0 + wave * 32;
  const bool active = q0 < N;
  stage_tile_f32<HD, 128>(Q + ((size_t)bh * N + qb0) * HD, HD, N - qb0, Qs);
  f32x16 oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) oacc[d][t] = 0.f;
  float ms = -1e30f, l = 0.f;
  for (int kt = 0; kt < (N + 63) / 64; ++kt) {
    __syncthreads();
    stage_tile_f32<HD, 64>(K + ((size_t)bh * N + kt * 64) * HD, HD, N - kt * 64, Ks);      // rows past N: zeros, masked below
    stage_tile_f32<HD, 64>(V + ((size_t)bh * N + kt * 64) * HD, HD, N - kt * 64, Vs);
    __syncthreads();
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int t = 0; t < 16; ++t) s[kb][t] = 0.f;
#pragma unroll 8
      for (int kk = 0; kk < HD; kk += 2) s[kb] = MFMA_F32(Ks[(kb * 32 + r) * LD + kk + h], Qs[(wave * 32 + r) * LD + kk + h], s[kb]);
      if (kt * 64 + 64 > N) mask_rows_past(s[kb], kt * 64 + kb * 32, h, N);
    }
    float mx = s[0][0];
#pragma unroll
    for (int t = 0; t < 16; ++t) mx = fmaxf(mx, fmaxf(s[0][t], s[1][t]));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float ms_new = fmaxf(ms, mx * c), alpha = exp2f(ms - ms_new);
    ms = ms_new;
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 16; ++t) { const float p = exp2f(s[kb][t] * c - ms); s[kb][t] = p; rs += p; }
    l = l * alpha + rs;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
#pragma unroll
      for (int t = 0; t < 16; ++t) oacc[d][t] *= alpha;
      const bool dv = d * 32 + r < HD;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const float a = dv ? Vs[(kb * 32 + acc_row(t, h)) * LD + d * 32 + r] : 0.f;
          oacc[d] = MFMA_F32(a, s[kb][t], oacc[d]);
        }
    }
  }
  l += __shfl_xor(l, 32, 64);
  if (!active) return;
  const float inv = 1.f / l;
  const int b = bh / H, hh = bh % H;
  float* op = O + ((size_t)(b * N + q0 + r) * H + hh) * HD;
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int dd = d * 32 + acc_row(t, h);
      if (dd < HD && q0 + r < N) op[dd] = oacc[d][t] * inv;
    }
  if (h == 0 && q0 + r < N) LSE[(size_t)bh * N + q0 + r] = (ms + log2f(l)) * 0.6931471805599453f;
}

// Head dim 16 (the VMAE heads: what `_encode` / `decode_to_images` run in the reference's f32): the 32x32x2 form above pads the P.V product to 32
// output rows (a third of its MFMA cycles wasted) and stages its tiles synchronously.  Here everything is 16x16x4 f32 MFMAs: S^T blocks
// [16 keys][16 queries] = K . Q^T (4 MFMAs per block, the 16 dims), and -- the accumulator-as-operand trick of the bf16 kernels in its 16x16
// form -- element r of a score block's accumulator IS the B operand of step r of O^T[16 dims][16 queries] += V^T . P with contraction slot
// g = key 4 g + r of the block; the A operand reads V[key][dim] from LDS.  A wave owns 32 queries (two column blocks that share every K / V
// read), tiles of 64 keys, the next tile's rows in flight in registers under the current tile's arithmetic.  Running maximum per tile
// as in the general kernel; the exponentials are the bare v_exp_f32 (arguments <= 0: what it flushes to zero lies below 2^-126 of the row maximum).
__global__ __launch_bounds__(256) void attn_fwd_f32_hd16_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                                float* __restrict__ O, float* __restrict__ LSE, int H, int N, float c, QkvLayout L) {
  constexpr int HD = 16, LD = 20;              // LDS row pitch in floats: 16-B aligned rows; both operand read patterns conflict-free (banks 20 key + g, 80 g + d)
  __shared__ __attribute__((aligned(16))) float Ks[2][64 * LD], Vs[2][64 * LD];      // double-buffered: one barrier per tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int qblocks = (N + 127) / 128;
  const int bh = blockIdx.x / qblocks, q0 = (blockIdx.x % qblocks) * 128 + wave * 32;
  const size_t hb = (size_t)(bh / H) * L.sb + (size_t)(bh % H) * L.sh;      // head-major [B,H,N,16] or the packed token-major qkv (QkvLayout)
  const long ld = L.ld;
  const float* kb = K + hb;
  const float* vb = V + hb;
  float qv[2][4];                              // Q[q0 + 16 qb + j][4 s + g] * c: the B operand of the score products
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) qv[qb][s4] = Q[hb + (size_t)min(q0 + 16 * qb + j, N - 1) * ld + 4 * s4 + g] * c;
  f32x4 oacc[2];
  float ms[2], l[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) { oacc[qb] = (f32x4){0.f, 0.f, 0.f, 0.f}; ms[qb] = -1e30f; l[qb] = 0.f; }
  const int nt = (N + 63) / 64;
  const int srow = threadIdx.x >> 2, sch = (threadIdx.x & 3) * 4;            // this thread's 16 B of every K and V tile
  auto fetch = [&](int kt, float4& kr, float4& vr) {
    const int row = kt * 64 + srow;
    if (row < N) { kr = *(const float4*)(kb + (size_t)row * ld + sch); vr = *(const float4*)(vb + (size_t)row * ld + sch); }
    else { kr = make_float4(0.f, 0.f, 0.f, 0.f); vr = kr; }                  // rows past N: zeros, masked below
  };
  float4 kr, vr;
  fetch(0, kr, vr);
  *(float4*)&Ks[0][srow * LD + sch] = kr;
  *(float4*)&Vs[0][srow * LD + sch] = vr;
  __syncthreads();
  if (nt > 1) fetch(1, kr, vr);                // tile kt + 1 waits in registers while tile kt is computed
  for (int kt = 0; kt < nt; ++kt) {
    const float* Kt = Ks[kt & 1];
    const float* Vt = Vs[kt & 1];
    f32x4 sc[2][4];                            // [query block][key block]: rows = keys 16 kb + 4 g + r, column = query j
#pragma unroll
    for (int kbk = 0; kbk < 4; ++kbk) {
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) sc[qb][kbk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const float a = Kt[(16 * kbk + j) * LD + 4 * s4 + g];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) sc[qb][kbk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, qv[qb][s4], sc[qb][kbk], 0, 0, 0);
      }
    }
    if (kt * 64 + 64 > N) {                    // ragged last tile: keys past N drop out of the softmax
#pragma unroll
      for (int kbk = 0; kbk < 4; ++kbk)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kt * 64 + 16 * kbk + 4 * g + r >= N) { sc[0][kbk][r] = -__builtin_inff(); sc[1][kbk][r] = -__builtin_inff(); }
    }
    float alpha[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float mx = sc[qb][0][0];
#pragma unroll
      for (int kbk = 0; kbk < 4; ++kbk)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[qb][kbk][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float ms_new = fmaxf(ms[qb], mx);
      alpha[qb] = EXP2(ms[qb] - ms_new);
      ms[qb] = ms_new;
      float rs = 0.f;
#pragma unroll
      for (int kbk = 0; kbk < 4; ++kbk)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float pp = EXP2(sc[qb][kbk][r] - ms_new); sc[qb][kbk][r] = pp; rs += pp; }
      l[qb] = l[qb] * alpha[qb] + rs;
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[qb][r] *= alpha[qb];
    }
#pragma unroll
    for (int kbk = 0; kbk < 4; ++kbk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = Vt[(16 * kbk + 4 * g + r) * LD + j];                  // V^T[dim j][slot g] of step r
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) oacc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sc[qb][kbk][r], oacc[qb], 0, 0, 0);
      }
    if (kt + 1 < nt) {                         // the other buffer was last read one tile ago, before the previous barrier
      *(float4*)&Ks[(kt + 1) & 1][srow * LD + sch] = kr;
      *(float4*)&Vs[(kt + 1) & 1][srow * LD + sch] = vr;
      __syncthreads();
      if (kt + 2 < nt) fetch(kt + 2, kr, vr);
    }
  }
  const int b = bh / H, hh = bh % H;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float lt = l[qb];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const int q = q0 + 16 * qb + j;
    if (q < N) {
      const float inv = 1.f / lt;              // rows of O^T in this lane: dims 4 g .. 4 g + 3 of query q
      *(float4*)(O + ((size_t)(b * N + q) * H + hh) * HD + 4 * g) = make_float4(oacc[qb][0] * inv, oacc[qb][1] * inv, oacc[qb][2] * inv, oacc[qb][3] * inv);
      if (g == 0) LSE[(size_t)bh * N + q] = (ms[qb] + log2f(lt)) * 0.6931471805599453f;
    }
  }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_f32_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                                const float* __restrict__ dO, const float* __restrict__ LSE,
                                                                const float* __restrict__ DELTA, float* __restrict__ dK, float* __restrict__ dV,
                                                                int H, int N, float scale) {
  constexpr int LD = HD + 1, DB = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ks = (float*)smem;            // [128][LD]
  float* Vs = Ks + 128 * LD;           // [128][LD]
  float* Qs = Vs + 128 * LD;           // [64][LD]
  float* dOs = Qs + 64 * LD;           // [64][LD]
  float* lse2 = dOs + 64 * LD;         // [64]
  float* dl = lse2 + 64;               // [64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const float c = scale * 1.4426950408889634f;
  const int kblocks = (N + 127) / 128;
  const int bh = blockIdx.x / kblocks, kb0 = (blockIdx.x % kblocks) * 128, k0 = kb0 + wave * 32;
  const bool active = k0 < N;
  const int b = bh / H, hh = bh % H;
  stage_tile_f32<HD, 128>(K + ((size_t)bh * N + kb0) * HD, HD, N - kb0, Ks);
  stage_tile_f32<HD, 128>(V + ((size_t)bh * N + kb0) * HD, HD, N - kb0, Vs);
  f32x16 dkacc[DB], dvacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) { dkacc[d][t] = 0.f; dvacc[d][t] = 0.f; }
  for (int qt = 0; qt < (N + 63) / 64; ++qt) {
    __syncthreads();
    stage_tile_f32<HD, 64>(Q + ((size_t)bh * N + qt * 64) * HD, HD, N - qt * 64, Qs);
    stage_tile_f32<HD, 64>(dO + (((size_t)b * N + qt * 64) * H + hh) * HD, (long)H * HD, N - qt * 64, dOs);
    // query rows past N: lse = +inf -> p = exp2(0 - inf) = 0, so they add nothing to dV or dK
    if (threadIdx.x < 64) lse2[threadIdx.x] = qt * 64 + (int)threadIdx.x < N ? LSE[(size_t)bh * N + qt * 64 + threadIdx.x] * 1.4426950408889634f : __builtin_inff();
    else if (threadIdx.x < 128) dl[threadIdx.x - 64] = qt * 64 + (int)threadIdx.x - 64 < N ? DELTA[(size_t)bh * N + qt * 64 + threadIdx.x - 64] : 0.f;
    __syncthreads();
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16 s, dp;
#pragma unroll
      for (int t = 0; t < 16; ++t) { s[t] = 0.f; dp[t] = 0.f; }
#pragma unroll 8
      for (int kk = 0; kk < HD; kk += 2) {
        s = MFMA_F32(Qs[(qb * 32 + r) * LD + kk + h], Ks[(wave * 32 + r) * LD + kk + h], s);
        dp = MFMA_F32(dOs[(qb * 32 + r) * LD + kk + h], Vs[(wave * 32 + r) * LD + kk + h], dp);
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int row = qb * 32 + acc_row(t, h);
        const float p = exp2f(s[t] * c - lse2[row]);
        s[t] = p;
        dp[t] = p * (dp[t] - dl[row]);
      }
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const bool dv = d * 32 + r < HD;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int row = qb * 32 + acc_row(t, h);
          dvacc[d] = MFMA_F32(dv ? dOs[row * LD + d * 32 + r] : 0.f, s[t], dvacc[d]);
          dkacc[d] = MFMA_F32(dv ? Qs[row * LD + d * 32 + r] : 0.f, dp[t], dkacc[d]);
        }
      }
    }
  }
  if (!active || k0 + r >= N) return;
  float* dkp = dK + ((size_t)bh * N + k0 + r) * HD;
  float* dvp = dV + ((size_t)bh * N + k0 + r) * HD;
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int dd = d * 32 + acc_row(t, h);
      if (dd < HD) { dkp[dd] = dkacc[d][t] * scale; dvp[dd] = dvacc[d][t]; }
    }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dq_f32_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                              const float* __restrict__ dO, const float* __restrict__ LSE,
                                                              const float* __restrict__ DELTA, float* __restrict__ dQ, int H, int N, float scale) {
  constexpr int LD = HD + 1, DB = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = (float*)smem;            // [128][LD]
  float* dOs = Qs + 128 * LD;          // [128][LD]
  float* Ks = dOs + 128 * LD;          // [64][LD]
  float* Vs = Ks + 64 * LD;            // [64][LD]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const float c = scale * 1.4426950408889634f;
  const int qblocks = (N + 127) / 128;
  const int bh = blockIdx.x / qblocks, qb0 = (blockIdx.x % qblocks) * 128, q0 = qb0 + wave * 32;
  const bool active = q0 < N;
  const int b = bh / H, hh = bh % H;
  const int qrow = min(q0 + r, N - 1);
  stage_tile_f32<HD, 128>(Q + ((size_t)bh * N + qb0) * HD, HD, N - qb0, Qs);
  stage_tile_f32<HD, 128>(dO + (((size_t)b * N + qb0) * H + hh) * HD, (long)H * HD, N - qb0, dOs);
  const float lse2 = LSE[(size_t)bh * N + qrow] * 1.4426950408889634f, dl = DELTA[(size_t)bh * N + qrow];
  f32x16 dqacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) dqacc[d][t] = 0.f;
  for (int kt = 0; kt < (N + 63) / 64; ++kt) {
    __syncthreads();
    stage_tile_f32<HD, 64>(K + ((size_t)bh * N + kt * 64) * HD, HD, N - kt * 64, Ks);
    stage_tile_f32<HD, 64>(V + ((size_t)bh * N + kt * 64) * HD, HD, N - kt * 64, Vs);
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 s, dp;
#pragma unroll
      for (int t = 0; t < 16; ++t) { s[t] = 0.f; dp[t] = 0.f; }
#pragma unroll 8
      for (int kk = 0; kk < HD; kk += 2) {
        s = MFMA_F32(Ks[(kb * 32 + r) * LD + kk + h], Qs[(wave * 32 + r) * LD + kk + h], s);
        dp = MFMA_F32(Vs[(kb * 32 + r) * LD + kk + h], dOs[(wave * 32 + r) * LD + kk + h], dp);
      }
      if (kt * 64 + 64 > N) mask_rows_past(s, kt * 64 + kb * 32, h, N);       // keys past N: p = 0
#pragma unroll
      for (int t = 0; t < 16; ++t) dp[t] = exp2f(s[t] * c - lse2) * (dp[t] - dl);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const bool dv = d * 32 + r < HD;
#pragma unroll
        for (int t = 0; t < 16; ++t)
          dqacc[d] = MFMA_F32(dv ? Ks[(kb * 32 + acc_row(t, h)) * LD + d * 32 + r] : 0.f, dp[t], dqacc[d]);
      }
    }
  }
  if (!active || q0 + r >= N) return;
  float* dqp = dQ + ((size_t)bh * N + q0 + r) * HD;
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int dd = d * 32 + acc_row(t, h);
      if (dd < HD) dqp[dd] = dqacc[d][t] * scale;
    }
}

// ================================================================================================ C ABI
// The head dims the kernels are instantiated for: f(IC<hd>{}) receives the head dim as a compile-time constant; any other is refused.
template <typename F> static int attn_hd_dispatch(int hd, F&& f) {                // the 16-bit kernels
  switch (hd) {
    case 16: f(IC<16>{}); break; case 32: f(IC<32>{}); break; case 64: f(IC<64>{}); break; case 72: f(IC<72>{}); break; case 128: f(IC<128>{}); break;
    default: LDMAE_FAIL(LDMAE_ERR_INVALID, "attention(bf16): head_dim %d unsupported (16, 32, 64, 72, 128)", hd);
  }
  return LDMAE_OK;
}
template <typename F> static int attn_hd_dispatch_f32(int hd, F&& f) {            // 80 / 96: mae_vit_huge's heads of 80 and anything up to 96 -- the f32 BACKWARD's LDS tiles do not fit at 128
  switch (hd) {
    case 16: f(IC<16>{}); break; case 32: f(IC<32>{}); break; case 64: f(IC<64>{}); break; case 72: f(IC<72>{}); break; case 80: f(IC<80>{}); break;
    case 96: f(IC<96>{}); break; case 128: f(IC<128>{}); break;
    default: LDMAE_FAIL(LDMAE_ERR_INVALID, "attention(f32): head_dim %d unsupported (16, 32, 64, 72, 80, 96, 128)", hd);
  }
  return LDMAE_OK;
}

// dynamic LDS of the bf16 kernels: the K/V (Q/dO) ring, and at least the 4 per-wave store images that re-use it at the end
static int attn_lds(int hd, int extra) {
  const int hdp = hd_pad(hd), ring = ATT_STAGES * (2 * 64 * hdp * 2 + extra), scratch = 4 * 32 * (hdp * 2 + 16);
  return ring > scratch ? ring : scratch;
}

// Operand-fragment prefetch depth (template parameter PF) of the backward kernels on whole tiles; ragged N runs depth 0.  Head dim 64: 1, in
// the fused pair (the B/1 step) bitwise equal to PF = 0 and 2-3 % faster, -2.4 % in the plain pair (profiles/r06_attn_prefetch_ab.txt).  Head
// dim 16 (the VMAE blocks' backward, bound by vector issue) measured NEUTRAL with it (1.225 vs 1.221 ms at 256 x 12 x 1024^2) and keeps
// 0, like head dim 128 (one wave per SIMD either way) and the head dims that were not measured.
constexpr int attn_pf(int hd) { return hd == 64 ? 1 : 0; }
// The depth to run.  Diagnostic build: tune keys 23 (fused dK/dV), 24 (fused dQ), 25 (the plain pair; value 2 has no instantiation there):
// 0 = the shipped depth, 1 / 2 = that depth, 3 = no prefetch (tools/bench_attn.py --prefetch, tools/bench_attn16.py --prefetch).
static int attn_pf_depth(int key, int hd) {
#ifdef LDMAE_DIAG
  const int t = ldmae_tune_get(key);
  if (t == 3) return 0;
  if (t == 1 || (t == 2 && key != 25)) return t;
#endif
  return attn_pf(hd);
}
// f(IC<pf>{}) for the depth chosen above.  The product library instantiates the shipped depth only.
template <int HD, int MAXPF, typename F> static void attn_pf_dispatch(int pf, F&& f) {
#ifdef LDMAE_DIAG
  if (pf == 0) return f(IC<0>{});
  if (pf == 1) return f(IC<1>{});
  if constexpr (MAXPF >= 2) return f(IC<2>{});
#endif
  f(IC<attn_pf(HD)>{});
}

// mult8: the entry point also requires hd % 8 == 0 (the 16-bit kernels move 16-B chunks of a row)
static int attn_check(const char* who, int dtype, int B, int H, int N, int hd, bool mult8 = false) {
  ldmae_count(dtype == LDMAE_F16 ? LDMAE_COUNT_ATTN_F16 : (dtype == LDMAE_BF16 ? LDMAE_COUNT_ATTN_BF16 : LDMAE_COUNT_ATTN_F32));
  LDMAE_REQUIRE(dtype == LDMAE_F32 || dtype == LDMAE_BF16 || dtype == LDMAE_F16, "%s: bad dtype %d", who, dtype);
  LDMAE_REQUIRE(B > 0 && H > 0 && N > 0 && hd > 0, "%s: empty problem", who);
  LDMAE_REQUIRE(!mult8 || hd % 8 == 0, "%s: head_dim %d must be a multiple of 8", who, hd);
  return LDMAE_OK;      // any N: the last 64-row tile of a sweep may be ragged (mask_rows_past)
}

static int attention_fwd_core(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int hd,
                              float scale, QkvLayout Lq, QkvLayout Lv, hipStream_t st, const float* score_bound = nullptr, int sb_heads = 0) {
  const unsigned grid = (unsigned)B * H * ((N + 127) / 128);
  const float c = scale * 1.4426950408889634f;
  // the 16-bit forward of head dim HD; R: the ragged instantiation (N % 64 != 0), F: fp16 operands
  auto fwd16 = [&](auto HD, auto R, auto F) {
    constexpr int hd_ = decltype(HD)::value;
    attn_launch(attn_fwd_bf16_kernel<hd_, decltype(R)::value != 0, decltype(F)::value != 0>, grid, attn_lds(hd_, 0), st, q, k, v, o, lse, H, N, c, Lq, Lv,
                score_bound, sb_heads);
  };
  if (dtype == LDMAE_F16) {
    // the TF32-class forward (fp16 operands): head_dim 16, the VMAE heads
    LDMAE_REQUIRE(hd == 16 && score_bound == nullptr, "attention_fwd(fp16): head_dim 16 only (the VMAE heads), no static bound");
    if (N % 64 == 0) fwd16(IC<16>{}, IC<0>{}, IC<1>{}); else fwd16(IC<16>{}, IC<1>{}, IC<1>{});
  } else if (dtype == LDMAE_BF16) {
    if (int e = attn_hd_dispatch(hd, [&](auto HD) { if (N % 64 == 0) fwd16(HD, IC<0>{}, IC<0>{}); else fwd16(HD, IC<1>{}, IC<0>{}); })) return e;
  } else {
    LDMAE_REQUIRE((hd == 16 && Lq.ld == Lv.ld && Lq.sh == Lv.sh && Lq.sb == Lv.sb) ||
                  (Lq.ld == hd && Lq.sh == (long)N * hd && Lv.ld == hd && Lv.sh == (long)N * hd),
                  "attention_fwd(f32): head-major q/k/v only (head_dim 16: also the packed qkv)");
    if (hd == 16) hipLaunchKernelGGL(attn_fwd_f32_hd16_kernel, dim3(grid), dim3(256), 0, st, (const float*)q, (const float*)k, (const float*)v, (float*)o, lse, H, N, c, Lq);
    else if (int e = attn_hd_dispatch_f32(hd, [&](auto HD) {
               constexpr int hd_ = decltype(HD)::value;
               attn_launch(attn_fwd_f32_kernel<hd_>, grid, (size_t)(128 + 64 + 64) * (hd_ + 1) * 4, st, q, k, v, o, lse, H, N, c);
             })) return e;
  }
  LDMAE_CHECK_LAUNCH("attention_fwd");
  return LDMAE_OK;
}

extern "C" int ldmae_attention_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int hd,
                                   float scale, void* stream) {
  LDMAE_REQUIRE(q && k && v && o && lse, "attention_fwd: null pointer");
  if (int e = attn_check("attention_fwd", dtype, B, H, N, hd)) return e;
  const QkvLayout hm = layout_hm(H, N, hd);
  return attention_fwd_core(dtype, q, k, v, o, lse, B, H, N, hd, scale, hm, hm, as_stream(stream));
}

extern "C" int ldmae_attention_fwd_qkv(int dtype, const void* qkv, void* o, float* lse, int B, int H, int N, int hd, float scale, void* stream) {
  LDMAE_REQUIRE(qkv && o && lse, "attention_fwd_qkv: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16 || ((dtype == LDMAE_F32 || dtype == LDMAE_F16) && hd == 16),
                "attention_fwd_qkv: bf16, or f32 / fp16 at head_dim 16 (other f32 head dims take head-major q/k/v)");
  if (int e = attn_check("attention_fwd_qkv", dtype, B, H, N, hd, true)) return e;
  const long hw = (long)H * hd;
  const QkvLayout pk = layout_pk(H, N, hd);
  if (dtype == LDMAE_F32) {
    const float* pf = (const float*)qkv;
    return attention_fwd_core(dtype, pf, pf + hw, pf + 2 * hw, o, lse, B, H, N, hd, scale, pk, pk, as_stream(stream));
  }
  const bf16* p = (const bf16*)qkv;
  return attention_fwd_core(dtype, p, p + hw, p + 2 * hw, o, lse, B, H, N, hd, scale, pk, pk, as_stream(stream));
}

// max_j |k_j|^2 per (batch, head) of a packed token-major qkv [B*N][3][H][hd] (bf16) -> out [B*H][2] = (0, max): the input of
// ldmae_attention_fwd_qkv_bounded when nothing upstream knows the norms (one pass over the k slots; worth it for long sequences only).
__global__ __launch_bounds__(256) void k_norm_max_kernel(const bf16* __restrict__ qkv, unsigned* __restrict__ out, int N, int H, int hd) {
  __shared__ unsigned hmax[64];
  const int b = blockIdx.y, t0 = blockIdx.x * 64;
  if (threadIdx.x < 64) hmax[threadIdx.x] = 0u;
  __syncthreads();
  const int pairs = min(64, N - t0) * H;
  for (int p = threadIdx.x; p < pairs; p += 256) {
    const int tok = t0 + p / H, hh = p % H;
    const bf16* kr = qkv + (((size_t)b * N + tok) * 3 + 1) * H * hd + (size_t)hh * hd;
    float ss = 0.f;
    for (int ch = 0; ch < hd / 8; ++ch) {
      const bf16x8 v = *(const bf16x8*)(kr + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += (float)v[j] * (float)v[j];
    }
    atomicMax(&hmax[hh], __float_as_uint(ss));           // non-negative floats order like their bits
  }
  __syncthreads();
  if (threadIdx.x < H) atomicMax(out + ((size_t)b * H + threadIdx.x) * 2 + 1, hmax[threadIdx.x]);
}
extern "C" int ldmae_k_norm_max(const void* qkv, float* qk_max2, int B, int N, int H, int hd, void* stream) {
  LDMAE_REQUIRE(qkv && qk_max2 && B > 0 && N > 0, "k_norm_max: null pointer or empty problem");
  LDMAE_REQUIRE(H >= 1 && H <= 64 && hd % 8 == 0, "k_norm_max: %d heads (1 .. 64) of %d (multiple of 8)", H, hd);
  // the atomic-max buffer MUST start at zero (a smaller-than-true maximum makes the static-shift softmax wrong, silently)
  LDMAE_REQUIRE(hipMemsetAsync(qk_max2, 0, (size_t)B * H * 2 * sizeof(float), as_stream(stream)) == hipSuccess, "k_norm_max: hipMemsetAsync of the norm buffer failed");
  hipLaunchKernelGGL(k_norm_max_kernel, dim3((N + 63) / 64, B), dim3(256), 0, as_stream(stream), (const bf16*)qkv, (unsigned*)qk_max2, N, H, hd);
  LDMAE_CHECK_LAUNCH("k_norm_max");
  return LDMAE_OK;
}

// ldmae_attention_fwd_qkv with the static softmax shift from per-(batch, head) norm maxima: qk_max2 [B*H][2] f32 on the device =
// (max_i |q_i|^2, max_j |k_j|^2) of the q / k rows as stored in the packed qkv.  Heads whose bound |q|max |k|max scale log2(e) * 1.02 exceeds 50
// keep the running maximum.  The maxima must be true maxima (or larger): a smaller value makes the result wrong.
extern "C" int ldmae_attention_fwd_qkv_bounded(int dtype, const void* qkv, void* o, float* lse, const float* qk_max2, int B, int H, int N, int hd,
                                               float scale, void* stream) {
  LDMAE_REQUIRE(qkv && o && lse && qk_max2, "attention_fwd_qkv_bounded: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16, "attention_fwd_qkv_bounded: bf16 only");
  if (int e = attn_check("attention_fwd_qkv_bounded", dtype, B, H, N, hd, true)) return e;
  const bf16* p = (const bf16*)qkv;
  const long hw = (long)H * hd;
  const QkvLayout pk = layout_pk(H, N, hd);
  return attention_fwd_core(dtype, p, p + hw, p + 2 * hw, o, lse, B, H, N, hd, scale, pk, pk, as_stream(stream), qk_max2, 1);
}

static int attention_bwd_core(int dtype, const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                              void* dq, void* dk, void* dv, float* delta, int B, int H, int N, int hd, float scale, QkvLayout Lq, QkvLayout Lv, hipStream_t st) {
  const unsigned grid = (unsigned)B * H * ((N + 127) / 128);
  // delta = [2][B*H*NP] f32 workspace, NP = N rounded up to 64 (bf16: -delta | -lse*log2e, rows padded to whole tiles; f32: slot 0 = delta, unpadded)
  const long items = (long)B * N * H, rcs = (long)B * H * ((N + 63) / 64 * 64);
  const unsigned dgrid = (unsigned)((items * 8 + 255) / 256 < 8192 ? (items * 8 + 255) / 256 : 8192);
  // The 16-bit pair of head dim HD; R: the ragged instantiations (N % 64 != 0), F: fp16 operands / gradients, P: prefetch depth.
  // dQ first: it forms delta = rowsum(dO * O) from its own fragments and publishes it for the dK/dV kernel
  auto pair16 = [&](auto HD, auto R, auto F, auto P) {
    constexpr int hd_ = decltype(HD)::value, pf = decltype(P)::value;
    constexpr bool r = decltype(R)::value != 0, f16 = decltype(F)::value != 0;
    attn_launch(attn_bwd_dq_bf16_kernel<hd_, false, r, f16, pf>, grid, attn_lds(hd_, 0), st, q, k, v, o, do_, lse, delta, rcs, dq, H, N, scale, Lq, Lv, QkNormBwd{});
    attn_launch(attn_bwd_dkdv_bf16_kernel<hd_, false, r, f16, pf>, grid, attn_lds(hd_, 1024), st, q, k, v, do_, delta, rcs, dk, dv, H, N, scale, Lq, Lv, QkNormBwd{});
  };
  // whole tiles: the depth of attn_pf_depth; ragged N: depth 0
  auto pair16_n = [&](auto HD, auto F) {
    constexpr int hd_ = decltype(HD)::value;
    if (N % 64 == 0) attn_pf_dispatch<hd_, 1>(attn_pf_depth(25, hd_), [&](auto P) { pair16(HD, IC<0>{}, F, P); });
    else pair16(HD, IC<1>{}, F, IC<0>{});
  };
  if (dtype == LDMAE_F16) {
    // fp16 operands / gradients (VMAE pre-training under fp16 autocast; head_dim 16): the bf16 kernels with the f16 MFMAs and conversions
    LDMAE_REQUIRE(hd == 16, "attention_bwd(fp16): head_dim 16 only (the VMAE heads)");
    pair16_n(IC<16>{}, IC<1>{});
  } else if (dtype == LDMAE_BF16) {
    if (int e = attn_hd_dispatch(hd, [&](auto HD) { pair16_n(HD, IC<0>{}); })) return e;
  } else {
    LDMAE_REQUIRE(Lq.ld == hd && Lq.sh == (long)N * hd && Lv.ld == hd && Lv.sh == (long)N * hd, "attention_bwd(f32): head-major q/k/v only");
    LDMAE_REQUIRE((size_t)(128 + 128 + 64 + 64) * (hd + 1) * 4 + 512 <= 160 * 1024,
                  "attention_bwd(f32): head_dim %d needs more than the 160 KiB of LDS (f32 backward: head dims up to 96; bf16 covers 128)", hd);
    hipLaunchKernelGGL(attn_delta_kernel<float>, dim3(dgrid), dim3(256), 0, st, (const float*)o, (const float*)do_, delta, B, H, N, hd);
    if (int e = attn_hd_dispatch_f32(hd, [&](auto HD) {
          constexpr int hd_ = decltype(HD)::value;
          constexpr size_t l1 = (size_t)(128 + 128 + 64 + 64) * (hd_ + 1) * 4 + 512;
          attn_launch(attn_bwd_dkdv_f32_kernel<hd_>, grid, l1, st, q, k, v, do_, lse, delta, dk, dv, H, N, scale);
          attn_launch(attn_bwd_dq_f32_kernel<hd_>, grid, l1, st, q, k, v, do_, lse, delta, dq, H, N, scale);
        })) return e;
  }
  LDMAE_CHECK_LAUNCH("attention_bwd");
  return LDMAE_OK;
}

extern "C" int ldmae_attention_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                                   void* dq, void* dk, void* dv, float* delta, int B, int H, int N, int hd, float scale, void* stream) {
  LDMAE_REQUIRE(q && k && v && o && do_ && lse && dq && dk && dv && delta, "attention_bwd: null pointer");
  if (int e = attn_check("attention_bwd", dtype, B, H, N, hd, true)) return e;
  const QkvLayout hm = layout_hm(H, N, hd);
  return attention_bwd_core(dtype, q, k, v, o, do_, lse, dq, dk, dv, delta, B, H, N, hd, scale, hm, hm, as_stream(stream));
}

extern "C" int ldmae_attention_bwd_qkv(int dtype, const void* qkv, const void* o, const void* do_, const float* lse, void* dqkv, float* delta,
                                       int B, int H, int N, int hd, float scale, void* stream) {
  LDMAE_REQUIRE(qkv && o && do_ && lse && dqkv && delta, "attention_bwd_qkv: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16 || (dtype == LDMAE_F16 && hd == 16), "attention_bwd_qkv: bf16, or fp16 at head_dim 16");
  if (int e = attn_check("attention_bwd_qkv", dtype, B, H, N, hd, true)) return e;
  const bf16* p = (const bf16*)qkv;
  bf16* g = (bf16*)dqkv;
  const long hw = (long)H * hd;
  const QkvLayout pk = layout_pk(H, N, hd);
  return attention_bwd_core(dtype, p, p + hw, p + 2 * hw, o, do_, lse, g, g + hw, g + 2 * hw, delta, B, H, N, hd, scale, pk, pk, as_stream(stream));
}

// q, k (dq, dk) head-major [B,H,N,hd]; v read from -- and dv written into -- the v slot of a packed token-major [B,N,3,H,hd] buffer
// (the LightningDiT block: QK-norm + RoPE produce new q / k, v is used exactly as the qkv Linear wrote it)
extern "C" int ldmae_attention_fwd_pv(int dtype, const void* q, const void* k, const void* qkv, void* o, float* lse, int B, int H, int N, int hd,
                                      float scale, void* stream) {
  LDMAE_REQUIRE(q && k && qkv && o && lse, "attention_fwd_pv: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16, "attention_fwd_pv: bf16 only");
  if (int e = attn_check("attention_fwd_pv", dtype, B, H, N, hd, true)) return e;
  const long hw = (long)H * hd;
  const QkvLayout hm = layout_hm(H, N, hd), pk = layout_pk(H, N, hd);
  return attention_fwd_core(dtype, q, k, (const bf16*)qkv + 2 * hw, o, lse, B, H, N, hd, scale, hm, pk, as_stream(stream));
}
// ldmae_attention_fwd_pv with a caller-supplied bound on |score * scale * log2(e)| (one float on the device; see the kernel): the softmax
// then runs with that static shift.  A bound that does not hold makes the result wrong (overflow), so it has to be a proven one.
extern "C" int ldmae_attention_fwd_pv_bounded(int dtype, const void* q, const void* k, const void* qkv, void* o, float* lse, const float* score_bound,
                                              int B, int H, int N, int hd, float scale, void* stream) {
  LDMAE_REQUIRE(q && k && qkv && o && lse && score_bound, "attention_fwd_pv_bounded: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16, "attention_fwd_pv_bounded: bf16 only");
  if (int e = attn_check("attention_fwd_pv_bounded", dtype, B, H, N, hd, true)) return e;
  const long hw = (long)H * hd;
  const QkvLayout hm = layout_hm(H, N, hd), pk = layout_pk(H, N, hd);
  return attention_fwd_core(dtype, q, k, (const bf16*)qkv + 2 * hw, o, lse, B, H, N, hd, scale, hm, pk, as_stream(stream), score_bound);
}
// The bound for heads that went through QK-RMSNorm + RoPE (lightningdit.py:66-80; qk_rope.hip: q = x * rsqrt(mean(x^2) + eps) * w, then a
// rotation): |q|^2 = sum w_i^2 xhat_i^2 <= max|w|^2 * hd, the same for k, RoPE preserves norms, so
// |q . k| * scale * log2(e) <= hd * max|wq| * max|wk| * scale * log2(e); 2 % on top for the bf16 roundings of q, k and of the scaled q.
__global__ void qk_score_bound_kernel(const float* __restrict__ wq, const float* __restrict__ wk, int hd, float c, float* __restrict__ out) {
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < hd; i += 64) { a = fmaxf(a, fabsf(wq[i])); b = fmaxf(b, fabsf(wk[i])); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a = fmaxf(a, __shfl_xor(a, o, 64)); b = fmaxf(b, __shfl_xor(b, o, 64)); }
  if (threadIdx.x == 0) out[0] = (float)hd * a * b * c * 1.02f;
}
extern "C" int ldmae_qk_score_bound(const float* wq, const float* wk, int hd, float scale, float* out, void* stream) {
  LDMAE_REQUIRE(wq && wk && out && hd > 0, "qk_score_bound: null pointer or empty head");
  hipLaunchKernelGGL(qk_score_bound_kernel, dim3(1), dim3(64), 0, as_stream(stream), wq, wk, hd, scale * 1.4426950408889634f, out);
  LDMAE_CHECK_LAUNCH("qk_score_bound");
  return LDMAE_OK;
}
extern "C" int ldmae_attention_bwd_pv(int dtype, const void* q, const void* k, const void* qkv, const void* o, const void* do_, const float* lse,
                                      void* dq, void* dk, void* dqkv, float* delta, int B, int H, int N, int hd, float scale, void* stream) {
  LDMAE_REQUIRE(q && k && qkv && o && do_ && lse && dq && dk && dqkv && delta, "attention_bwd_pv: null pointer");
  LDMAE_REQUIRE(dtype == LDMAE_BF16, "attention_bwd_pv: bf16 only");
  if (int e = attn_check("attention_bwd_pv", dtype, B, H, N, hd, true)) return e;
  const long hw = (long)H * hd;
  const QkvLayout hm = layout_hm(H, N, hd), pk = layout_pk(H, N, hd);
  return attention_bwd_core(dtype, q, k, (const bf16*)qkv + 2 * hw, o, do_, lse, dq, dk, (bf16*)dqkv + 2 * hw, delta, B, H, N, hd, scale, hm, pk,
                            as_stream(stream));
}

// ---- attention backward + QK-RMSNorm / RoPE backward in one (LightningDiT block, bf16): dq / dk never exist head-major; the packed dqkv
// comes out complete (q | k through the norm / rope backward in the epilogues, v as attention_bwd_pv), with the norm-weight gradients
// and the qkv bias gradient.  Replaces ldmae_attention_bwd_pv + ldmae_qknorm_rope_bwd for head dims 64 / 128.
extern "C" long ldmae_attention_bwd_pv_qknorm_workspace_bytes(int B, int H, int N, int hd) {
  const long blk = (long)B * ((N + 127) / 128);
  const long cw = ldmae_colsum_workspace_bytes((int)(blk * H), 2 * hd), cb = ldmae_colsum_workspace_bytes((int)blk, 3 * H * hd);
  const long cmax = ((cw > cb ? cw : cb) + 15) / 16 * 16;
  return (2L * B * H * N + blk * H * 2 * hd + blk * 3 * H * hd + 2L * hd) * 4 + cmax;
}
extern "C" int ldmae_attention_bwd_pv_qknorm(int dtype, const void* q, const void* k, const void* qkv, const void* o, const void* do_,
                                             const float* lse, const float* wq, const float* wk, const float* cos, const float* sin, float eps,
                                             void* dqkv, float* dwq, float* dwk, float* dbias, float* workspace, int B, int H, int N, int hd,
                                             float scale, void* stream) {
  LDMAE_REQUIRE(q && k && qkv && o && do_ && lse && cos && sin && dqkv && dbias && workspace, "attention_bwd_pv_qknorm: null pointer");
  LDMAE_REQUIRE(!wq == !wk && (!wq || (dwq && dwk)), "attention_bwd_pv_qknorm: pass wq, wk, dwq, dwk (QK-norm + RoPE) or none of them (RoPE only: use_qknorm=False)");
  LDMAE_REQUIRE(dtype == LDMAE_BF16, "attention_bwd_pv_qknorm: bf16 only");
  LDMAE_REQUIRE(hd == 64 || hd == 128, "attention_bwd_pv_qknorm: head_dim %d (64 or 128; others: attention_bwd_pv + qknorm_rope_bwd)", hd);
  if (int e = attn_check("attention_bwd_pv_qknorm", dtype, B, H, N, hd)) return e;
  LDMAE_REQUIRE(N % 64 == 0, "attention_bwd_pv_qknorm: N=%d must be a multiple of 64 (ragged N: attention_bwd_pv + qknorm_rope_bwd)", N);
  hipStream_t st = as_stream(stream);
  const long hw = (long)H * hd, items = (long)B * H * N, blk = (long)B * ((N + 127) / 128);
  const QkvLayout hm = layout_hm(H, N, hd), pk = layout_pk(H, N, hd);
  float* rowc = workspace;
  float* Pw = rowc + 2 * items;
  float* Pb = Pw + blk * H * 2 * hd;
  float* dw2 = Pb + blk * 3 * H * hd;              // [2*hd] = dwq | dwk
  float* cws = dw2 + 2 * hd;
  const QkNormBwd qn{(const bf16*)qkv, wq, wk, cos, sin, (bf16*)dqkv, Pw, Pb, eps};
  const unsigned grid = (unsigned)B * H * ((N + 127) / 128);
  const bf16* v = (const bf16*)qkv + 2 * hw;
  bf16* dv = (bf16*)dqkv + 2 * hw;
  // dQ first, as in attention_bwd_core; whole tiles only (N % 64 == 0, above)
  auto fused = [&](auto HD) {
    constexpr int hd_ = decltype(HD)::value;
    attn_pf_dispatch<hd_, 2>(attn_pf_depth(24, hd_), [&](auto P) {
      attn_launch(attn_bwd_dq_bf16_kernel<hd_, true, false, false, decltype(P)::value>, grid, attn_lds(hd_, 0), st, q, k, v, o, do_, lse, rowc, items, nullptr, H, N,
                  scale, hm, pk, qn);
    });
    attn_pf_dispatch<hd_, 2>(attn_pf_depth(23, hd_), [&](auto P) {
      attn_launch(attn_bwd_dkdv_bf16_kernel<hd_, true, false, false, decltype(P)::value>, grid, attn_lds(hd_, 1024), st, q, k, v, do_, rowc, items, nullptr, dv, H, N,
                  scale, hm, pk, qn);
    });
  };
  if (hd == 64) fused(IC<64>{}); else fused(IC<128>{});
  LDMAE_CHECK_LAUNCH("attention_bwd_pv_qknorm");
  if (!wq) {}                   // RoPE only: no norm-weight gradients
  else if (dwk == dwq + hd) {        // the caller keeps dwq | dwk adjacent: reduce straight into them
    if (int e = ldmae_colsum(LDMAE_F32, Pw, 2 * hd, (int)(blk * H), 2 * hd, dwq, 0.f, cws, stream)) return e;
  } else {
    if (int e = ldmae_colsum(LDMAE_F32, Pw, 2 * hd, (int)(blk * H), 2 * hd, dw2, 0.f, cws, stream)) return e;
    hipMemcpyAsync(dwq, dw2, hd * sizeof(float), hipMemcpyDeviceToDevice, st);
    hipMemcpyAsync(dwk, dw2 + hd, hd * sizeof(float), hipMemcpyDeviceToDevice, st);
  }
  return ldmae_colsum(LDMAE_F32, Pb, 3 * (int)hw, (int)blk, 3 * (int)hw, dbias, 0.f, cws, stream);
}
