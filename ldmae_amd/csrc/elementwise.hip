// HBM-bound row kernels of the LightningDiT block (gfx950, wave64): RMSNorm / LayerNorm + modulate, forward and backward, and the
// gated-residual backward.  (QK-norm / RoPE: qk_rope.hip; SwiGLU, column sums, casts, thin GEMMs, embedders, AdamW: pointwise.hip.)
// One wave per row for the norm kernels (12 elements per lane at D = 768, shuffles for the row reduce); per-sample and per-column gradient
// sums are two-stage (per-workgroup partial rows, then a fixed-order reduce) so results are bitwise reproducible run to run.
#include "rowwise_common.h"

// out[o*out_ld + c] = beta*out + sum_{r<group} P[(o*group + r)*p_ld + c]; 8 row-lanes per column stride the group,
// partial sums are combined in a fixed order (bitwise reproducible).
template <int RL>
__global__ __launch_bounds__(32 * RL) void group_reduce_kernel(const float* __restrict__ P, int p_ld, int nout, int cols, int group,
                                                              float* __restrict__ out, int out_ld, float beta,
                                                              const float* __restrict__ P2 = nullptr, float* __restrict__ out2 = nullptr,
                                                              float beta2 = 0.f) {
  __shared__ float red[RL][33];
  if (blockIdx.z == 1) { P = P2; out = out2; beta = beta2; }        // a second reduction of the same shape in the same launch
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, o = blockIdx.y;
  float s = 0.f;
  if (c < cols) {
    const float* p = P + (size_t)o * group * p_ld + c;
    for (int r = rl; r < group; r += RL) s += p[(size_t)r * p_ld];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) {
    float t = red[0][cl];
#pragma unroll
    for (int k = 1; k < RL; ++k) t += red[k][cl];
    float* q = out + (size_t)o * out_ld + c;
    *q = (beta != 0.f ? beta * *q : 0.f) + t;
  }
}
void group_reduce(const float* P, int p_ld, int nout, int cols, int group, float* out, int out_ld, float beta, hipStream_t st,
                  const float* P2, float* out2, float beta2) {      // (declared, with the defaults, in rowwise_common.h)
  // long groups (thousands of per-workgroup partial rows into one output row): 32 row lanes, otherwise 8.  P2 / out2: a second reduction
  // of the same shape rides in the same launch (grid z = 2), with exactly the arithmetic it would have on its own
  const unsigned gz = P2 ? 2 : 1;
  if (group >= 256)
    hipLaunchKernelGGL(group_reduce_kernel<32>, dim3(cdiv(cols, 32), nout, gz), dim3(1024), 0, st, P, p_ld, nout, cols, group, out, out_ld, beta, P2, out2, beta2);
  else
    hipLaunchKernelGGL(group_reduce_kernel<8>, dim3(cdiv(cols, 32), nout, gz), dim3(256), 0, st, P, p_ld, nout, cols, group, out, out_ld, beta, P2, out2, beta2);
}

// ------------------------------------------------------------------ RMSNorm + modulate
// FULL (D % 256 == 0, M % 16 == 0, rows_per_batch % 16 == 0: the workgroup's 16 rows belong to one sample): no per-chunk guards, and the
// per-sample (1 + scale) / shift vectors are loaded ONCE per wave before the row loop.  The guarded form re-loads them per row and chunk
// behind a branch and a full `s_waitcnt vmcnt(0)` each: six serialized L2 round trips in the middle of every row.
// (A variant with all four rows of a wave requested up front -- 12 loads in flight per lane, 100 VGPRs -- measured 3 % SLOWER than one row
// at a time: here the waves in flight carry the bandwidth.)
template <int NCH, typename OutT, bool FULL = false>
__global__ __launch_bounds__(256) void rmsnorm_mod_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ shift, const float* __restrict__ scale,
                                                              int mod_ld, OutT* __restrict__ out, float* __restrict__ rstd, int M, int D,
                                                              int rpb, float eps, int center = 0) {
#define NORM_EMIT(m, a, b, y) store4<OutT>(out + (size_t)(m) * D + (a) + (b), y)
#include "norm_mod_rows.inc"
#undef NORM_EMIT
}

// x^2 + y^2 + z^2 + w^2 with the roundings the GUARDED form of rmsnorm_mod_fwd_kernel has.  Its `ss += hsum(xv * xv)` sits in a loop of
// conditional loads, one basic block per chunk, and is contracted there as fma(x, x, y * y) + fma(z, z, w * w) -- except with a single chunk
// (NCH == 1), where the products are formed as a packed multiply and nothing is contracted.  A kernel that forms the row in registers has
// another block structure and would get another contraction (1 ulp in rstd), so the guarded form of the residual + norm kernel spells the
// roundings out.  (The unguarded forms of the two kernels have the same structure and compile to the same sequence; both are covered
// bitwise by tests/test_gpu_resnorm_fused.py.)
template <bool FMA> __device__ __forceinline__ float sumsq4_guarded(float4 a) {
#pragma clang fp contract(off)
  if constexpr (FMA) return fmaf(a.x, a.x, a.y * a.y) + fmaf(a.z, a.z, a.w * a.w);
  else return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
}

// The gated residual(s) in front of the norm, formed in registers: r = gate_res4(x, gate_a[b], ya), then r = gate_res4(r, gate_b[b], yb) when
// yb is given (the second residual of a block, whose first was never stored).  r is written to xout (f32) and / or normalised + modulated into
// `out` exactly as rmsnorm_mod_fwd_kernel does with a row it loads: same row-to-wave mapping, same order of the sum of squares, same output
// arithmetic, following norm_mod_rows.inc statement for statement (its load half and sumsq4_guarded differ by design, so it does not
// include that text) -- xout / out / rstd have the bits of the EPI_GATE_RES epilogue followed by that kernel.  ya / yb are the
// branch outputs AS STORED in the activation type (what the epilogue adds).  Everything a row needs from HBM is requested before its first use.
template <int NCH, typename T, bool FULL = false>
__global__ __launch_bounds__(256) void res_rmsnorm_mod_fwd_kernel(const float* __restrict__ x, const T* __restrict__ ya,
                                                                  const float* __restrict__ ga, int ga_ld, const T* __restrict__ yb,
                                                                  const float* __restrict__ gb, int gb_ld, float* __restrict__ xout,
                                                                  const float* __restrict__ w, const float* __restrict__ shift,
                                                                  const float* __restrict__ scale, int mod_ld, T* __restrict__ out,
                                                                  float* __restrict__ rstd, int M, int D, int rpb, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = D >> 2;
  float4 wv[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) { const int c = lane + 64 * i; wv[i] = (c < nch && out) ? *(const float4*)(w + 4 * c) : f4(0.f); }
  if constexpr (FULL) {
    const int m0 = (blockIdx.x * 4 + wave) * 4, b = m0 / rpb;
    float4 sc1[NCH], sh[NCH], gav[NCH], gbv[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      sc1[i] = scale ? f4(1.f) + *(const float4*)(scale + (size_t)b * mod_ld + 4 * lane + 256 * i) : f4(1.f);
      sh[i] = shift ? *(const float4*)(shift + (size_t)b * mod_ld + 4 * lane + 256 * i) : f4(0.f);
      gav[i] = *(const float4*)(ga + (size_t)b * ga_ld + 4 * lane + 256 * i);
      gbv[i] = yb ? *(const float4*)(gb + (size_t)b * gb_ld + 4 * lane + 256 * i) : f4(0.f);
    }
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + r;
      const size_t ro = (size_t)m * D + 4 * lane;
      float4 xv[NCH], yav[NCH], ybv[NCH];
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) xv[i] = *(const float4*)(x + ro + 256 * i);
#pragma unroll
      for (int i = 0; i < NCH; ++i) { yav[i] = load4<T>(ya + ro + 256 * i); ybv[i] = yb ? load4<T>(yb + ro + 256 * i) : f4(0.f); }
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        xv[i] = gate_res4(xv[i], gav[i], yav[i]);
        if (yb) xv[i] = gate_res4(xv[i], gbv[i], ybv[i]);
        if (xout) *(float4*)(xout + ro + 256 * i) = xv[i];
      }
      if (!out) continue;
#pragma unroll
      for (int i = 0; i < NCH; ++i) ss += hsum(xv[i] * xv[i]);
      ss = wave_sum(ss);
      const float rs = rsqrtf(ss / (float)D + eps);
      if (lane == 0 && rstd) rstd[m] = rs;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        float4 y = (xv[i] * rs) * wv[i];
        if (scale) y = y * sc1[i];
        if (shift) y = y + sh[i];
        store4<T>(out + ro + 256 * i, y);
      }
    }
    return;
  }
  for (int r = 0; r < 4; ++r) {
    const int m = (blockIdx.x * 4 + wave) * 4 + r;
    if (m >= M) return;
    const int b = m / rpb;
    float4 xv[NCH], yav[NCH], ybv[NCH];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      xv[i] = c < nch ? *(const float4*)(x + (size_t)m * D + 4 * c) : f4(0.f);
      yav[i] = c < nch ? load4<T>(ya + (size_t)m * D + 4 * c) : f4(0.f);
      ybv[i] = (c < nch && yb) ? load4<T>(yb + (size_t)m * D + 4 * c) : f4(0.f);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        xv[i] = gate_res4(xv[i], *(const float4*)(ga + (size_t)b * ga_ld + 4 * c), yav[i]);
        if (yb) xv[i] = gate_res4(xv[i], *(const float4*)(gb + (size_t)b * gb_ld + 4 * c), ybv[i]);
        if (xout) *(float4*)(xout + (size_t)m * D + 4 * c) = xv[i];
      }
      ss += sumsq4_guarded<(NCH > 1)>(xv[i]);
    }
    if (!out) continue;
    ss = wave_sum(ss);
    const float rs = rsqrtf(ss / (float)D + eps);
    if (lane == 0 && rstd) rstd[m] = rs;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float4 y = (xv[i] * rs) * wv[i];
        if (scale) y = y * (f4(1.f) + *(const float4*)(scale + (size_t)b * mod_ld + 4 * c));
        if (shift) y = y + *(const float4*)(shift + (size_t)b * mod_ld + 4 * c);
        store4<T>(out + (size_t)m * D + 4 * c, y);
      }
    }
  }
}

// ------------------------------------------------------------------ shared by the backward row kernels
// a float4 AS STORED in the activation type: rounded to T and widened again
template <typename T> __device__ __forceinline__ float4 as_stored(float4 d) {
  return make_float4(to_f<T>(from_f<T>(d.x)), to_f<T>(from_f<T>(d.y)), to_f<T>(from_f<T>(d.z)), to_f<T>(from_f<T>(d.w)));
}
// The gated-residual backward of four channels of one row, written once for gate_bwd_kernel and for the GATE tail of rmsnorm_mod_bwd_kernel
// (which promises that kernel's bits): g is the gradient of the residual stream, gv the gate, y4 the expression that loads the branch output
// (evaluated only where the gate gradient is wanted).  acc_g += g * y;  dy = g * gate, rounded to T and stored;  acc_b += dy AS STORED --
// the bias gradient of the Linear that produced the branch = column sums of dy as the weight-gradient GEMM reads it, formed here while the
// values are in registers instead of inside the TN GEMM.  mul_rn: never contracted into the bias sum.
#define GATE_BWD_TAIL(T, want_g, want_b, acc_g, acc_b, g, y4, gv, dyp) do { \
    if (want_g) acc_g = acc_g + (g) * (y4); \
    const float4 d_ = mul_rn(g, gv); \
    store4<T>(dyp, d_); \
    if (want_b) acc_b = acc_b + as_stored<T>(d_); \
  } while (0)
// The flush of a workgroup's accumulators into its partial row(s).  WAVE_SETS_TO_LDS(WAVE_SET(N, 0, a) ... WAVE_SET(N, N - 1, z)): the N
// per-wave accumulator sets go to LDS as red[wave][set][D] (a lane holds columns 4 * (lane + 64 * i) .. + 3 of chunk i), then a barrier;
// WAVE_SETS_SUM(N, k, i) is element i of set k summed over the four waves in the fixed order (w0 + w1) + (w2 + w3).  Macros over the
// kernel's own red / lane / wave / nch / D: as __forceinline__ functions they changed the compiled code of every kernel that used them
// (register allocation, and the descriptor of the wide ones), and these kernels are pinned to each other bitwise.
#define WAVE_SET(N, k, acc) *(float4*)(red + (wave * N + k) * D + 4 * c) = acc[i];
#define WAVE_SETS_TO_LDS(SETS) do { \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) { const int c = lane + 64 * i; if (c < nch) { SETS } } \
    __syncthreads(); \
  } while (0)
#define WAVE_SETS_SUM(N, k, i) ((red[(k) * D + (i)] + red[(N + (k)) * D + (i)]) + (red[(2 * N + (k)) * D + (i)] + red[(3 * N + (k)) * D + (i)]))

// partials P[wg][3][D] = {sum dout, sum dout*y, sum dy*n} over the workgroup's rows (one sample)
// GATE: the gated-residual backward of the branch BELOW this norm (the attention branch under norm2) rides along: the updated residual
// gradient is consumed while it is in registers -- dy = dx_new * gate[b] (rounded to T), dgate partials sum dx_new * y, bias-gradient
// partials sum dy -- instead of being re-read by a separate gate_bwd pass (805 MB per block).  Same arithmetic, same partial layout
// and same summation order as gate_bwd_kernel: both use GATE_BWD_TAIL and the WAVE_SETS_* flush above.
// RECOMP (GATE only): `x` is the residual stream BEFORE the gated residual under this norm and the row that was normalised is rebuilt in
// registers, gate_res4(x, gate[b], y) -- the very expression that formed it in the forward (res_rmsnorm_mod_fwd_kernel) -- from the y row and
// the gate constants this kernel reads anyway: that row never has to be stored.  Only the source of the f32 row changes.
struct GateBwdArgs { const void* y; const float* gate; int gate_ld; void* dy; float* Pg; float* Pb; int dx_overwrite; int center; int recompute; };
template <int NCH, typename T, bool GATE, bool FULL = false, bool RECOMP = false>
__global__ __launch_bounds__(256) void rmsnorm_mod_bwd_kernel(const T* __restrict__ dout, const float* __restrict__ x,
                                                              const float* __restrict__ w, const float* __restrict__ scale, int mod_ld,
                                                              const float* __restrict__ rstd, float* __restrict__ dx, float* __restrict__ P,
                                                              int M, int D, int rpb, int rows_per_wg, GateBwdArgs ga) {
  extern __shared__ float red[];   // [4 waves][3][D]; GATE: the first 3*D floats hold the per-column constants during the row loop
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = D >> 2;
  const int m_base = blockIdx.x * rows_per_wg, b = m_base / rpb;
  float4 wv[GATE ? 1 : NCH], sc1[GATE ? 1 : NCH], a_sh[NCH], a_sc[NCH], a_w[NCH];
  float4 a_g[GATE ? NCH : 1], a_b[GATE ? NCH : 1];
  const T* gy = (const T*)ga.y;
  T* gdy = (T*)ga.dy;
  // GATE: five accumulator sets live in registers, so the three per-column constants (norm weight, 1 + scale, gate) are kept in LDS
  // and re-read per row instead (36 registers: 174 -> 3 waves per SIMD instead of 2 for a kernel that lives on bytes in flight)
  float* cw = red;
  float* cs = red + D;
  float* cg = red + 2 * D;
  if constexpr (GATE) {
    for (int c = threadIdx.x; c < nch; c += 256) {
      *(float4*)(cw + 4 * c) = w ? *(const float4*)(w + 4 * c) : f4(1.f);
      *(float4*)(cs + 4 * c) = scale ? f4(1.f) + *(const float4*)(scale + (size_t)b * mod_ld + 4 * c) : f4(1.f);
      *(float4*)(cg + 4 * c) = *(const float4*)(ga.gate + (size_t)b * ga.gate_ld + 4 * c);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if constexpr (!GATE) {
      wv[i] = c < nch ? (w ? *(const float4*)(w + 4 * c) : f4(1.f)) : f4(0.f);
      sc1[i] = (c < nch && scale) ? f4(1.f) + *(const float4*)(scale + (size_t)b * mod_ld + 4 * c) : f4(1.f);
    }
    a_sh[i] = a_sc[i] = a_w[i] = f4(0.f);
    if constexpr (GATE) a_g[i] = a_b[i] = f4(0.f);
  }
  if constexpr (FULL) {
    // D == NCH * 256 (host): no per-chunk guards, and everything a row needs from HBM -- dout, x, the old dx and (GATE) y -- is requested
    // before the first use: 4 * NCH loads in flight per lane.  (The guarded form below compiles to one branch + `s_waitcnt vmcnt(0)` per
    // chunk: 2 loads in flight.)  Per-element arithmetic and summation order are those of the guarded form.
    for (int r = wave; r < rows_per_wg; r += 4) {
      const int m = m_base + r;
      if (m >= M) break;
      const size_t ro = (size_t)m * D + 4 * lane;
      float4 g[NCH], nv[NCH], dold[NCH], yv[GATE ? NCH : 1];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        g[i] = load4<T>(dout + ro + 256 * i); nv[i] = *(const float4*)(x + ro + 256 * i);
        if constexpr (RECOMP) yv[i] = load4<T>(gy + ro + 256 * i);          // needed before the first use of nv: with the first batch
      }
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        dold[i] = ga.dx_overwrite ? f4(0.f) : *(const float4*)(dx + ro + 256 * i);
        if constexpr (GATE && !RECOMP) yv[i] = load4<T>(gy + ro + 256 * i);
      }
      const float rs = rstd[m];
      float4 dn[NCH];
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        const float4 wc = GATE ? *(const float4*)(cw + 4 * c) : wv[i], sc = GATE ? *(const float4*)(cs + 4 * c) : sc1[i];
        if constexpr (RECOMP) nv[i] = gate_res4(nv[i], *(const float4*)(cg + 4 * c), yv[i]);
        nv[i] = nv[i] * rs;
        const float4 dy = g[i] * sc;
        a_sh[i] = a_sh[i] + g[i];
        a_sc[i] = a_sc[i] + g[i] * (nv[i] * wc);
        a_w[i] = a_w[i] + dy * nv[i];
        dn[i] = dy * wc;
        dot += hsum(dn[i] * nv[i]);
      }
      dot = wave_sum_dpp(dot) / (float)D;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        const float4 d0 = (dn[i] - nv[i] * dot) * rs;
        const float4 gn = ga.dx_overwrite ? d0 : dold[i] + d0;
        *(float4*)(dx + ro + 256 * i) = gn;
        if constexpr (GATE) GATE_BWD_TAIL(T, true, true, a_g[i], a_b[i], gn, yv[i], *(const float4*)(cg + 4 * c), gdy + ro + 256 * i);
      }
    }
  } else
  for (int r = wave; r < rows_per_wg; r += 4) {
    const int m = m_base + r;
    if (m >= M) break;
    const float rs = rstd[m];
    float4 nv[NCH], dn[NCH];
    float dot = 0.f, mean = 0.f;
    // center (LayerNorm without affine parameters: the norm of the CENTRED row): the row mean is recomputed from x (a second, cache-resident
    // read), n = (x - mean) * rstd, and the centring's own backward takes the mean of dn out of the result below.  mean = msum = 0 otherwise:
    // x - 0 and d - 0 leave every bit of the RMS form as it was.
    if (ga.center) {
      float s1 = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) { const int c = lane + 64 * i; if (c < nch) s1 += hsum(*(const float4*)(x + (size_t)m * D + 4 * c)); }
      mean = wave_sum(s1) / (float)D;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        const float4 g = load4<T>(dout + (size_t)m * D + 4 * c);
        const float4 wc = GATE ? *(const float4*)(cw + 4 * c) : wv[i], sc = GATE ? *(const float4*)(cs + 4 * c) : sc1[i];
        float4 xr = *(const float4*)(x + (size_t)m * D + 4 * c);
        if constexpr (RECOMP) xr = gate_res4(xr, *(const float4*)(cg + 4 * c), load4<T>(gy + (size_t)m * D + 4 * c));
        nv[i] = (xr - f4(mean)) * rs;
        const float4 dy = g * sc;
        a_sh[i] = a_sh[i] + g;
        a_sc[i] = a_sc[i] + g * (nv[i] * wc);
        a_w[i] = a_w[i] + dy * nv[i];
        dn[i] = dy * wc;
        dot += hsum(dn[i] * nv[i]);
      } else { nv[i] = dn[i] = f4(0.f); }
    }
    dot = wave_sum(dot) / (float)D;
    float msum = 0.f;
    if (ga.center) {
      float s1 = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) s1 += hsum(dn[i]);
      msum = wave_sum(s1) / (float)D;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float* p = dx + (size_t)m * D + 4 * c;
        const float4 d0 = ((dn[i] - nv[i] * dot) - f4(msum)) * rs;
        const float4 g = ga.dx_overwrite ? d0 : *(const float4*)p + d0;        // beta_x = 0: dx is written, not read (no memset by the caller)
        *(float4*)p = g;
        if constexpr (GATE)
          GATE_BWD_TAIL(T, true, true, a_g[i], a_b[i], g, load4<T>(gy + (size_t)m * D + 4 * c), *(const float4*)(cg + 4 * c), gdy + (size_t)m * D + 4 * c);
      }
    }
  }
  if constexpr (GATE) __syncthreads();            // every wave is done with the constants: the region becomes reduction scratch
  WAVE_SETS_TO_LDS(WAVE_SET(3, 0, a_sh) WAVE_SET(3, 1, a_sc) WAVE_SET(3, 2, a_w));
  for (int i = threadIdx.x; i < 3 * D; i += 256) P[(size_t)blockIdx.x * 3 * D + i] = WAVE_SETS_SUM(3, 0, i);
  if constexpr (GATE) {
    __syncthreads();
    WAVE_SETS_TO_LDS(WAVE_SET(2, 0, a_g) WAVE_SET(2, 1, a_b));
    for (int i = threadIdx.x; i < D; i += 256) {
      ga.Pg[(size_t)blockIdx.x * D + i] = WAVE_SETS_SUM(2, 0, i);
      ga.Pb[(size_t)blockIdx.x * D + i] = WAVE_SETS_SUM(2, 1, i);
    }
  }
}

// per-sample reduce of the per-workgroup partials, every set optional: P [G][3][D] -> dshift / dscale [B, dmod_ld] and dwb [B, D] (the norm
// weight gradient per sample); Pg [G][D] -> dgate [B, dgate_ld]; Pb [G][D] -> dbb [B, D] (the bias gradient per sample).  One launch for
// what used to be a reduce kernel + a grouped reduce + the first stage of a column sum; dwb and dbb are then summed over the samples by
// ONE group_reduce launch (grid z = 2).
__global__ void mod_partials_reduce_kernel(const float* __restrict__ P, int D, int gps, float* __restrict__ dshift,
                                           float* __restrict__ dscale, int dmod_ld, float* __restrict__ dwb,
                                           const float* __restrict__ Pg = nullptr, float* __restrict__ dgate = nullptr, int dgate_ld = 0,
                                           const float* __restrict__ Pb = nullptr, float* __restrict__ dbb = nullptr) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (d >= D) return;
  // The partials of a sample are added in their fixed order (bitwise equal to the stand-alone gate_bwd path), but LOADED eight at a time: the
  // rolled loop had one load in flight per accumulator and the launch was a chain of dependent L2 round trips (29 us for 31 MB)
  auto sum = [&](const float* p, size_t stride) {
    float s = 0.f;
    int g = 0;
    for (; g + 8 <= gps; g += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(g + j) * stride];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; g < gps; ++g) s += p[(size_t)g * stride];
    return s;
  };
  if (P) {
    const float* p = P + (size_t)b * gps * 3 * D + d;
    const float s0 = sum(p, (size_t)3 * D), s1 = sum(p + D, (size_t)3 * D), s2 = sum(p + 2 * D, (size_t)3 * D);
    if (dshift) dshift[(size_t)b * dmod_ld + d] = s0;
    if (dscale) dscale[(size_t)b * dmod_ld + d] = s1;
    dwb[(size_t)b * D + d] = s2;
  }
  if (Pg) dgate[(size_t)b * dgate_ld + d] = sum(Pg + (size_t)b * gps * D + d, (size_t)D);
  if (Pb) dbb[(size_t)b * D + d] = sum(Pb + (size_t)b * gps * D + d, (size_t)D);
}

static int norm_modulate_fwd(int out_dtype, const float* x, const float* w, const float* shift, const float* scale,
                             int mod_ld, void* out, float* rstd, int M, int D, int rows_per_batch, float eps, int center, void* stream) {
  LDMAE_REQUIRE(x && (w || center) && out && M > 0 && D > 0, "rmsnorm_modulate_fwd: null pointer or empty");
  LDMAE_REQUIRE(D % 4 == 0 && (mod_ld % 4 == 0 || (!shift && !scale)), "rmsnorm_modulate_fwd: D=%d mod_ld=%d must be multiples of 4", D, mod_ld);
  LDMAE_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0, "rmsnorm_modulate_fwd: M=%d %% rows_per_batch=%d != 0", M, rows_per_batch);
  hipStream_t st = as_stream(stream);
  const unsigned grid = cdiv(M, 16);
  const bool full = D % 256 == 0 && M % 16 == 0 && rows_per_batch % 16 == 0 && !center;       // bf16 only
  int rc = LDMAE_OK;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    rc = row_nch_dispatch(D, [&](auto nch) {
      constexpr int NCH = decltype(nch)::value;
      if constexpr (__is_same(T, bf16)) if (full) { hipLaunchKernelGGL((rmsnorm_mod_fwd_kernel<NCH, bf16, true>), dim3(grid), dim3(256), 0, st, x, w, shift, scale, mod_ld, (bf16*)out, rstd, M, D, rows_per_batch, eps, 0); return; }
      hipLaunchKernelGGL((rmsnorm_mod_fwd_kernel<NCH, T>), dim3(grid), dim3(256), 0, st, x, w, shift, scale, mod_ld, (T*)out, rstd, M, D, rows_per_batch, eps, center);
    });
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(out_dtype, go)), "%s: dtype %d (f32 or bf16)", center ? "layernorm_modulate_fwd" : "rmsnorm_modulate_fwd", out_dtype);
  if (rc) return rc;
  LDMAE_CHECK_LAUNCH("rmsnorm_modulate_fwd");
  return LDMAE_OK;
}
extern "C" int ldmae_rmsnorm_modulate_fwd(int out_dtype, const float* x, const float* w, const float* shift, const float* scale,
                                          int mod_ld, void* out, float* rstd, int M, int D, int rows_per_batch, float eps, void* stream) {
  return norm_modulate_fwd(out_dtype, x, w, shift, scale, mod_ld, out, rstd, M, D, rows_per_batch, eps, 0, stream);
}
// r = x + gate_a[b] * ya (+ gate_b[b] * yb when yb is given); xout = r (optional); out / rstd = rmsnorm_modulate_fwd of r (optional; at least
// one of xout / out).  dtype: the 16-bit activation type of ya / yb / out.
extern "C" int ldmae_res_rmsnorm_modulate_fwd(int dtype, const float* x, const void* ya, const float* gate_a, int gate_a_ld, const void* yb,
                                              const float* gate_b, int gate_b_ld, float* xout, const float* w, const float* shift,
                                              const float* scale, int mod_ld, void* out, float* rstd, int M, int D, int rows_per_batch, float eps,
                                              void* stream) {
  LDMAE_REQUIRE(dtype == LDMAE_BF16 || dtype == LDMAE_F16, "res_rmsnorm_modulate_fwd: dtype %d (bf16 or fp16 activations only)", dtype);
  LDMAE_REQUIRE(x && ya && gate_a && (xout || out) && M > 0 && D > 0, "res_rmsnorm_modulate_fwd: null pointer or empty");
  LDMAE_REQUIRE((yb != nullptr) == (gate_b != nullptr), "res_rmsnorm_modulate_fwd: yb and gate_b go together");
  LDMAE_REQUIRE(!out || w, "res_rmsnorm_modulate_fwd: the norm needs its weight");
  LDMAE_REQUIRE(out || (!rstd && !shift && !scale), "res_rmsnorm_modulate_fwd: rstd / shift / scale without a norm output");
  LDMAE_REQUIRE(xout != x, "res_rmsnorm_modulate_fwd: xout must not alias x");
  LDMAE_REQUIRE(D % 4 == 0 && gate_a_ld % 4 == 0 && (!yb || gate_b_ld % 4 == 0) && (mod_ld % 4 == 0 || (!shift && !scale)),
                "res_rmsnorm_modulate_fwd: D=%d gate_ld=%d/%d mod_ld=%d must be multiples of 4", D, gate_a_ld, gate_b_ld, mod_ld);
  LDMAE_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0, "res_rmsnorm_modulate_fwd: M=%d %% rows_per_batch=%d != 0", M, rows_per_batch);
  const uintptr_t al = (uintptr_t)x | (uintptr_t)ya | (uintptr_t)gate_a | (uintptr_t)yb | (uintptr_t)gate_b | (uintptr_t)xout | (uintptr_t)w |
                       (uintptr_t)shift | (uintptr_t)scale | (uintptr_t)out;
  LDMAE_REQUIRE(al % 16 == 0, "res_rmsnorm_modulate_fwd: every tensor must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const unsigned grid = cdiv(M, 16);
  // (fp16 keeps the guarded form: ldmae_rmsnorm_modulate_fwd has no fp16 output, and the f32 output it is compared with runs the guarded form)
  const bool full = D % 256 == 0 && M % 16 == 0 && rows_per_batch % 16 == 0;
  int rc = LDMAE_OK;
  dtype_dispatch<bf16, f16>(dtype, [&](auto t) {        // (codes outside the two were refused above)
    using T = tag_t<decltype(t)>;
    rc = row_nch_dispatch(D, [&](auto nch) {
      constexpr int NCH = decltype(nch)::value;
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, x, (const T*)ya, gate_a, gate_a_ld, (const T*)yb, gate_b, gate_b_ld, xout, w, shift, scale, mod_ld, (T*)out, rstd, M, D, rows_per_batch, eps); };
      if constexpr (__is_same(T, bf16)) if (full) return launch(res_rmsnorm_mod_fwd_kernel<NCH, bf16, true>);
      launch(res_rmsnorm_mod_fwd_kernel<NCH, T, false>);
    });
  });
  if (rc) return rc;
  LDMAE_CHECK_LAUNCH("res_rmsnorm_modulate_fwd");
  return LDMAE_OK;
}
// LayerNorm(elementwise_affine=False) + modulate: the norm of the blocks built with use_rmsnorm=False (lightningdit.py:200-201,257; eps 1e-6).
// rstd [M] = rsqrt(var + eps) (the backward recomputes the row mean from x).
extern "C" int ldmae_layernorm_modulate_fwd(int out_dtype, const float* x, const float* shift, const float* scale, int mod_ld, void* out,
                                            float* rstd, int M, int D, int rows_per_batch, float eps, void* stream) {
  return norm_modulate_fwd(out_dtype, x, nullptr, shift, scale, mod_ld, out, rstd, M, D, rows_per_batch, eps, 1, stream);
}

extern "C" long ldmae_rmsnorm_modulate_bwd_workspace_bytes(int M, int D, int rows_per_batch) {
  const int rw = pick_rows_per_wg(rows_per_batch);
  if (rw == 0) return -1;
  return ((long)(M / rw) * 3 * D + (long)(M / rows_per_batch) * D) * 4;
}


// What the five backward entries hand to rmsnorm_modulate_bwd_core, by name (w / dw null + center: the LayerNorm form; gated: ga.y / gate /
// gate_ld / dy and dgate / dgate_ld / dbias are set, by norm_bwd_gate_args)
struct NormBwdArgs {
  int dtype; const void* dout; const float* x; const float* w; const float* scale; int mod_ld; const float* rstd;
  float* dx_accum; float beta_x; float* dshift; float* dscale; int dmod_ld; float* dw; float beta_w;
  int M, D, rows_per_batch; float* workspace; void* stream; int center;
  bool gated; GateBwdArgs ga; float* dgate; int dgate_ld; float* dbias;
};
static int rmsnorm_modulate_bwd_core(const NormBwdArgs& a) {
  const int dtype = a.dtype, M = a.M, D = a.D, rows_per_batch = a.rows_per_batch, center = a.center;
  const bool gate = a.gated;
  float* dw = a.dw;
  LDMAE_REQUIRE(a.dout && a.x && (a.w || center) && a.rstd && a.dx_accum && (dw || center) && a.workspace, "rmsnorm_modulate_bwd: null pointer");
  LDMAE_REQUIRE(D % 4 == 0 && M > 0 && rows_per_batch > 0 && M % rows_per_batch == 0, "rmsnorm_modulate_bwd: bad shape M=%d D=%d rpb=%d", M, D, rows_per_batch);
  const int rw = pick_rows_per_wg(rows_per_batch);
  LDMAE_REQUIRE(rw > 0, "rmsnorm_modulate_bwd: rows_per_batch=%d must be a multiple of 4", rows_per_batch);
  hipStream_t st = as_stream(a.stream);
  const int G = M / rw, B = M / rows_per_batch, gps = rows_per_batch / rw;
  float* P = a.workspace;
  float* dwb = a.workspace + (size_t)G * 3 * D;
  float* gws = dwb + (size_t)B * D;                     // gate partials (fused form): [G][D] dgate, [G][D] bias, colsum scratch
  const size_t lds = (size_t)4 * 3 * D * sizeof(float);
  LDMAE_REQUIRE(a.beta_x == 0.f || a.beta_x == 1.f, "rmsnorm_modulate_bwd: beta_x must be 0 (write dx) or 1 (accumulate into dx)");
  GateBwdArgs ga = a.ga;
  if (gate) { ga.Pg = gws; ga.Pb = gws + (size_t)G * D; }
  ga.dx_overwrite = a.beta_x == 0.f;
  ga.center = center;
  if (center && !dw) dw = P;             // LayerNorm without affine parameters: no weight gradient; the last reduce (stream-ordered behind the consumers of P) writes its [D] sums there
  const bool recomp = gate && ga.recompute, full = D % 256 == 0 && !center;                 // both bf16 only
  LDMAE_REQUIRE(!recomp || (dtype == LDMAE_BF16 && !center), "rmsnorm_modulate_bwd_gate_recompute: bf16 activations and the RMSNorm form only");
  int rc = LDMAE_OK;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    rc = row_nch_dispatch(D, [&](auto nch) {
      constexpr int NCH = decltype(nch)::value;
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(G), dim3(256), lds, st, (const T*)a.dout, a.x, a.w, a.scale, a.mod_ld, a.rstd, a.dx_accum, P, M, D, rows_per_batch, rw, ga); };
      if constexpr (__is_same(T, bf16)) {
        if (recomp) { if (full) launch(rmsnorm_mod_bwd_kernel<NCH, bf16, true, true, true>); else launch(rmsnorm_mod_bwd_kernel<NCH, bf16, true, false, true>); return; }
        if (full) { if (gate) launch(rmsnorm_mod_bwd_kernel<NCH, bf16, true, true>); else launch(rmsnorm_mod_bwd_kernel<NCH, bf16, false, true>); return; }
      }
      if (gate) launch(rmsnorm_mod_bwd_kernel<NCH, T, true>); else launch(rmsnorm_mod_bwd_kernel<NCH, T, false>);
    });
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "%s%s: dtype %d (f32 or bf16)", center ? "layernorm_modulate_bwd" : "rmsnorm_modulate_bwd", gate ? "_gate" : "", dtype);
  if (rc) return rc;
  LDMAE_CHECK_LAUNCH("rmsnorm_modulate_bwd");
  if (gate) {        // two launches: every per-sample sum, then dw and dbias over the samples together
    float* dbb = ga.Pb + (size_t)G * D;                 // [B][D], behind the gate partials (ldmae_gate_bwd_workspace_bytes reserves it)
    hipLaunchKernelGGL(mod_partials_reduce_kernel, dim3(cdiv(D, 256), B), dim3(256), 0, st, P, D, gps, a.dshift, a.dscale, a.dmod_ld, dwb,
                       (const float*)ga.Pg, a.dgate, a.dgate_ld, (const float*)ga.Pb, dbb);
    group_reduce(dwb, D, 1, D, B, dw, D, a.beta_w, st, dbb, a.dbias, 0.f);
    LDMAE_CHECK_LAUNCH("rmsnorm_modulate_bwd_gate reduce");
    return LDMAE_OK;
  }
  hipLaunchKernelGGL(mod_partials_reduce_kernel, dim3(cdiv(D, 256), B), dim3(256), 0, st, P, D, gps, a.dshift, a.dscale, a.dmod_ld, dwb);
  group_reduce(dwb, D, 1, D, B, dw, D, a.beta_w, st);
  LDMAE_CHECK_LAUNCH("rmsnorm_modulate_bwd reduce");
  return LDMAE_OK;
}
// the gate half of the three "_gate" entries: their two refusals, in the entry's name, then the fields
static int norm_bwd_gate_args(NormBwdArgs& a, const char* entry, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                              int dgate_ld, float* dbias) {
  LDMAE_REQUIRE(y && gate && dy && dgate && dbias, "%s: null pointer", entry);
  LDMAE_REQUIRE(gate_ld % 4 == 0, "%s: gate_ld=%d must be a multiple of 4", entry, gate_ld);
  a.gated = true;
  a.ga.y = y; a.ga.gate = gate; a.ga.gate_ld = gate_ld; a.ga.dy = dy;
  a.dgate = dgate; a.dgate_ld = dgate_ld; a.dbias = dbias;
  return LDMAE_OK;
}

extern "C" int ldmae_rmsnorm_modulate_bwd(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                                          const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, float* dw,
                                          float beta_w, int M, int D, int rows_per_batch, float* workspace, void* stream) {
  NormBwdArgs a{};
  a.dtype = dtype; a.dout = dout; a.x = x; a.scale = scale; a.mod_ld = mod_ld; a.rstd = rstd; a.dx_accum = dx_accum; a.beta_x = beta_x;
  a.dshift = dshift; a.dscale = dscale; a.dmod_ld = dmod_ld; a.M = M; a.D = D; a.rows_per_batch = rows_per_batch;
  a.workspace = workspace; a.stream = stream;
  a.w = w; a.dw = dw; a.beta_w = beta_w;
  return rmsnorm_modulate_bwd_core(a);
}

extern "C" long ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes(int M, int D, int rows_per_batch) {
  const long a = ldmae_rmsnorm_modulate_bwd_workspace_bytes(M, D, rows_per_batch), b = ldmae_gate_bwd_workspace_bytes(M, D, rows_per_batch);
  return a < 0 ? a : a + b;
}
// rmsnorm_modulate_bwd followed by gate_bwd of the updated dx_accum (dy = dx_accum * gate[b] in `dtype`; dgate [B, dgate_ld] = sum_n
// dx_accum * y; dbias [D] = column sums of dy) in one pass over the rows.
extern "C" int ldmae_rmsnorm_modulate_bwd_gate(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                                               const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, float* dw,
                                               float beta_w, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                                               int dgate_ld, float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream) {
  NormBwdArgs a{};
  a.dtype = dtype; a.dout = dout; a.x = x; a.scale = scale; a.mod_ld = mod_ld; a.rstd = rstd; a.dx_accum = dx_accum; a.beta_x = beta_x;
  a.dshift = dshift; a.dscale = dscale; a.dmod_ld = dmod_ld; a.M = M; a.D = D; a.rows_per_batch = rows_per_batch;
  a.workspace = workspace; a.stream = stream;
  a.w = w; a.dw = dw; a.beta_w = beta_w;
  if (int rc = norm_bwd_gate_args(a, "rmsnorm_modulate_bwd_gate", y, gate, gate_ld, dy, dgate, dgate_ld, dbias)) return rc;
  return rmsnorm_modulate_bwd_core(a);
}
// ldmae_rmsnorm_modulate_bwd_gate for a norm whose input row was never stored: `x` is the residual stream BEFORE the gated residual under
// the norm and the kernel rebuilds the normalised row as x + gate[b] * y (RECOMP above).  Every output has the bits ldmae_rmsnorm_modulate_bwd_gate
// produces when it is handed that row materialised.  bf16 only.
extern "C" int ldmae_rmsnorm_modulate_bwd_gate_recompute(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                                                         const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld,
                                                         float* dw, float beta_w, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                                                         int dgate_ld, float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream) {
  NormBwdArgs a{};
  a.dtype = dtype; a.dout = dout; a.x = x; a.scale = scale; a.mod_ld = mod_ld; a.rstd = rstd; a.dx_accum = dx_accum; a.beta_x = beta_x;
  a.dshift = dshift; a.dscale = dscale; a.dmod_ld = dmod_ld; a.M = M; a.D = D; a.rows_per_batch = rows_per_batch;
  a.workspace = workspace; a.stream = stream;
  a.w = w; a.dw = dw; a.beta_w = beta_w;
  if (int rc = norm_bwd_gate_args(a, "rmsnorm_modulate_bwd_gate_recompute", y, gate, gate_ld, dy, dgate, dgate_ld, dbias)) return rc;
  a.ga.recompute = 1;
  return rmsnorm_modulate_bwd_core(a);
}
// The LayerNorm(elementwise_affine=False) forms of the two entry points above (use_rmsnorm=False blocks): same arguments without w / dw, same
// workspaces (ldmae_rmsnorm_modulate_bwd(_gate)_workspace_bytes).
extern "C" int ldmae_layernorm_modulate_bwd(int dtype, const void* dout, const float* x, const float* scale, int mod_ld, const float* rstd,
                                            float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, int M, int D, int rows_per_batch,
                                            float* workspace, void* stream) {
  NormBwdArgs a{};
  a.dtype = dtype; a.dout = dout; a.x = x; a.scale = scale; a.mod_ld = mod_ld; a.rstd = rstd; a.dx_accum = dx_accum; a.beta_x = beta_x;
  a.dshift = dshift; a.dscale = dscale; a.dmod_ld = dmod_ld; a.M = M; a.D = D; a.rows_per_batch = rows_per_batch;
  a.workspace = workspace; a.stream = stream;
  a.center = 1;
  return rmsnorm_modulate_bwd_core(a);
}
extern "C" int ldmae_layernorm_modulate_bwd_gate(int dtype, const void* dout, const float* x, const float* scale, int mod_ld, const float* rstd,
                                                 float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, const void* y, const float* gate,
                                                 int gate_ld, void* dy, float* dgate, int dgate_ld, float* dbias, int M, int D, int rows_per_batch,
                                                 float* workspace, void* stream) {
  NormBwdArgs a{};
  a.dtype = dtype; a.dout = dout; a.x = x; a.scale = scale; a.mod_ld = mod_ld; a.rstd = rstd; a.dx_accum = dx_accum; a.beta_x = beta_x;
  a.dshift = dshift; a.dscale = dscale; a.dmod_ld = dmod_ld; a.M = M; a.D = D; a.rows_per_batch = rows_per_batch;
  a.workspace = workspace; a.stream = stream;
  a.center = 1;
  if (int rc = norm_bwd_gate_args(a, "layernorm_modulate_bwd_gate", y, gate, gate_ld, dy, dgate, dgate_ld, dbias)) return rc;
  return rmsnorm_modulate_bwd_core(a);
}

// ------------------------------------------------------------------ gated residual backward
template <int NCH, typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ dxo, const T* __restrict__ y, const float* __restrict__ gate,
                                                       int gate_ld, T* __restrict__ dy, float* __restrict__ P, float* __restrict__ Pb,
                                                       int M, int D, int rpb, int rows_per_wg) {
  extern __shared__ float red[];   // [4][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = D >> 2;
  const int m_base = blockIdx.x * rows_per_wg, b = m_base / rpb;
  float4 gv[NCH], acc[NCH], accb[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    gv[i] = (c < nch && gate) ? *(const float4*)(gate + (size_t)b * gate_ld + 4 * c) : f4(1.f);
    acc[i] = f4(0.f); accb[i] = f4(0.f);
  }
  for (int r = wave; r < rows_per_wg; r += 4) {
    const int m = m_base + r;
    if (m >= M) break;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        const float4 g = *(const float4*)(dxo + (size_t)m * D + 4 * c);
        GATE_BWD_TAIL(T, P, Pb, acc[i], accb[i], g, load4<T>(y + (size_t)m * D + 4 * c), gv[i], dy + (size_t)m * D + 4 * c);
      }
    }
  }
  if (P) {
    WAVE_SETS_TO_LDS(WAVE_SET(1, 0, acc));
    for (int i = threadIdx.x; i < D; i += 256) P[(size_t)blockIdx.x * D + i] = WAVE_SETS_SUM(1, 0, i);
    __syncthreads();
  }
  if (Pb) {
    WAVE_SETS_TO_LDS(WAVE_SET(1, 0, accb));
    for (int i = threadIdx.x; i < D; i += 256) Pb[(size_t)blockIdx.x * D + i] = WAVE_SETS_SUM(1, 0, i);
  }
}
extern "C" long ldmae_gate_bwd_workspace_bytes(int M, int D, int rows_per_batch) {
  const int rw = pick_rows_per_wg(rows_per_batch);
  if (rw <= 0) return 0;
  const int G = M / rw;                                // dgate partials + bias-gradient partials + max(column-sum scratch, per-sample bias sums)
  const long tail = ldmae_colsum_workspace_bytes(G, D), dbb = (long)(M / rows_per_batch) * D * 4;
  return 2L * G * D * 4 + (tail > dbb ? tail : dbb);
}
extern "C" int ldmae_gate_bwd(int dtype, const float* dxout, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                              int dgate_ld, float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream) {
  LDMAE_REQUIRE(dxout && dy && M > 0 && D % 4 == 0, "gate_bwd: null pointer or D=%d not a multiple of 4", D);
  LDMAE_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0, "gate_bwd: M=%d %% rows_per_batch=%d != 0", M, rows_per_batch);
  LDMAE_REQUIRE(!dgate || (y && gate && workspace), "gate_bwd: dgate requested without y/gate/workspace");
  LDMAE_REQUIRE(!dbias || workspace, "gate_bwd: dbias requested without workspace");
  const int rw = pick_rows_per_wg(rows_per_batch);
  LDMAE_REQUIRE(rw > 0, "gate_bwd: rows_per_batch=%d must be a multiple of 4", rows_per_batch);
  hipStream_t st = as_stream(stream);
  const int G = M / rw;
  float* P = dgate ? workspace : nullptr;
  float* Pb = dbias ? workspace + (size_t)G * D : nullptr;
  const size_t lds = (size_t)4 * D * sizeof(float);
  int rc = LDMAE_OK;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    rc = row_nch_dispatch(D, [&](auto nch) { hipLaunchKernelGGL((gate_bwd_kernel<decltype(nch)::value, T>), dim3(G), dim3(256), lds, st, dxout, (const T*)y, gate, gate_ld, (T*)dy, P, Pb, M, D, rows_per_batch, rw); });
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "gate_bwd: dtype %d (f32 or bf16)", dtype);
  if (rc) return rc;
  LDMAE_CHECK_LAUNCH("gate_bwd");
  if (dgate && dbias) {      // the same two reduce launches, in the same order of summation, as the fused rmsnorm_modulate_bwd_gate (bitwise equal)
    const int B = M / rows_per_batch;
    float* dbb = Pb + (size_t)G * D;
    hipLaunchKernelGGL(mod_partials_reduce_kernel, dim3(cdiv(D, 256), B), dim3(256), 0, st, (const float*)nullptr, D, rows_per_batch / rw,
                       (float*)nullptr, (float*)nullptr, 0, (float*)nullptr, (const float*)P, dgate, dgate_ld, (const float*)Pb, dbb);
    group_reduce(dbb, D, 1, D, B, dbias, D, 0.f, st);
    LDMAE_CHECK_LAUNCH("gate_bwd reduce");
    return LDMAE_OK;
  }
  if (dgate) group_reduce(P, D, M / rows_per_batch, D, rows_per_batch / rw, dgate, dgate_ld, 0.f, st);
  if (dbias) return ldmae_colsum(LDMAE_F32, Pb, D, G, D, dbias, 0.f, Pb + (size_t)G * D, stream);   // two-stage column sum of the G partial rows
  LDMAE_CHECK_LAUNCH("gate_bwd reduce");
  return LDMAE_OK;
}
