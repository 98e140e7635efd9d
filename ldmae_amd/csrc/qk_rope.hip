// QK-RMSNorm + RoPE + head-major relayout of the packed qkv (forward and backward), and the stand-alone RoPE (gfx950, wave64).
#include "rowwise_common.h"

// ------------------------------------------------------------------ QK-RMSNorm + RoPE + head-major relayout
// item = (b, n, h); LPR lanes per item, 4 elements per lane.
// (rope_apply: common.h -- shared with the fused qkv epilogue of gemm_nt_common.h)
__device__ __forceinline__ float4 rope_apply_bwd(float4 g, float4 c, float4 s) {
  return make_float4(g.x * c.x + g.y * s.y, g.y * c.y - g.x * s.x, g.z * c.z + g.w * s.w, g.w * c.w - g.z * s.z);
}

template <int LPR, typename T>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ wq,
                                                              const float* __restrict__ wk, const float* __restrict__ cosT,
                                                              const float* __restrict__ sinT, T* __restrict__ q, T* __restrict__ k,
                                                              T* __restrict__ v, int B, int N, int H, int hd, float eps) {
  const int sub = threadIdx.x % LPR, c4 = sub * 4;
  const bool act = c4 < hd;
  const long items = (long)B * N * H;
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / LPR, gstride = (long)gridDim.x * 256 / LPR;
  const bool plain = cosT == nullptr;    // VMAE attention: head-major relayout only (models_mae.py:133-134)
  const bool norm = wq != nullptr;       // false with tables: RoPE only (use_qknorm=False: q_norm = k_norm = nn.Identity, lightningdit.py:60-61)
  const float4 wqv = (act && norm) ? *(const float4*)(wq + c4) : f4(1.f), wkv = (act && norm) ? *(const float4*)(wk + c4) : f4(1.f);
  for (long it = gid; it < items; it += gstride) {
    const int h = it % H, n = (it / H) % N, b = it / ((long)H * N);
    const T* src = qkv + ((size_t)(b * N + n) * 3 * H + h) * hd + c4;
    const size_t dst = ((size_t)(b * H + h) * N + n) * hd + c4;
    float4 qv = f4(0.f), kv = f4(0.f), vv = f4(0.f), cs = f4(0.f), sn = f4(0.f);
    if (act) {
      qv = load4<T>(src); kv = load4<T>(src + (size_t)H * hd);
      if (v) vv = load4<T>(src + (size_t)2 * H * hd);
      if (!plain) { cs = *(const float4*)(cosT + (size_t)n * hd + c4); sn = *(const float4*)(sinT + (size_t)n * hd + c4); }
    }
    if (plain) {
      if (act) { store4<T>(q + dst, qv); store4<T>(k + dst, kv); store4<T>(v + dst, vv); }
      continue;
    }
    const float rq = norm ? rsqrtf(group_sum<LPR>(hsum(qv * qv)) / (float)hd + eps) : 1.f;
    const float rk = norm ? rsqrtf(group_sum<LPR>(hsum(kv * kv)) / (float)hd + eps) : 1.f;
    if (act) {
      store4<T>(q + dst, rope_apply((qv * rq) * wqv, cs, sn));
      store4<T>(k + dst, rope_apply((kv * rk) * wkv, cs, sn));
      if (v) store4<T>(v + dst, vv);            // v == NULL: attention reads v from the packed qkv itself (ldmae_attention_fwd_pv)
    }
  }
}

// bf16, head dims 64 / 128: 8 elements = 16 B per lane and access (the 4-element form above moves 8 B per lane for bf16: half-width
// requests at 0.54-0.70x the 16-B rate, MI355X_MICROARCH), 8 / 16 lanes per item, two items in flight per lane group.
template <int LPR>
__global__ __launch_bounds__(256) void qknorm_rope_fwd8_kernel(const bf16* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                                               const float* __restrict__ cosT, const float* __restrict__ sinT, bf16* __restrict__ q,
                                                               bf16* __restrict__ k, int B, int N, int H, float eps) {
  constexpr int hd = LPR * 8;
  const int sub = threadIdx.x % LPR, c8 = sub * 8;
  const long items = (long)B * N * H;
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / LPR, gstride = (long)gridDim.x * 256 / LPR;
  float wqv[8], wkv[8];
  const bool norm = wq != nullptr;       // false: RoPE only (use_qknorm=False); x * 1 * 1 is exact
#pragma unroll
  for (int j = 0; j < 8; ++j) { wqv[j] = norm ? wq[c8 + j] : 1.f; wkv[j] = norm ? wk[c8 + j] : 1.f; }
  auto one = [&](long it, bf16x8 qi, bf16x8 ki) {
    const int h = it % H, n = (it / H) % N, b = it / ((long)H * N);
    const float4 c0 = *(const float4*)(cosT + (size_t)n * hd + c8), c1 = *(const float4*)(cosT + (size_t)n * hd + c8 + 4);
    const float4 s0 = *(const float4*)(sinT + (size_t)n * hd + c8), s1 = *(const float4*)(sinT + (size_t)n * hd + c8 + 4);
    float qv[8], kv[8], sq = 0.f, sk = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { qv[j] = (float)qi[j]; kv[j] = (float)ki[j]; }
    // same association as the 4-element form: (x0^2 + x1^2) + (x2^2 + x3^2) per 4-chunk, chunks summed by the lane-group butterfly
    sq = ((qv[0] * qv[0] + qv[1] * qv[1]) + (qv[2] * qv[2] + qv[3] * qv[3])) + ((qv[4] * qv[4] + qv[5] * qv[5]) + (qv[6] * qv[6] + qv[7] * qv[7]));
    sk = ((kv[0] * kv[0] + kv[1] * kv[1]) + (kv[2] * kv[2] + kv[3] * kv[3])) + ((kv[4] * kv[4] + kv[5] * kv[5]) + (kv[6] * kv[6] + kv[7] * kv[7]));
    const float rq = norm ? rsqrtf(group_sum<LPR>(sq) / (float)hd + eps) : 1.f, rk = norm ? rsqrtf(group_sum<LPR>(sk) / (float)hd + eps) : 1.f;
    const float4 a0 = rope_apply(make_float4(qv[0] * rq * wqv[0], qv[1] * rq * wqv[1], qv[2] * rq * wqv[2], qv[3] * rq * wqv[3]), c0, s0);
    const float4 a1 = rope_apply(make_float4(qv[4] * rq * wqv[4], qv[5] * rq * wqv[5], qv[6] * rq * wqv[6], qv[7] * rq * wqv[7]), c1, s1);
    const float4 b0 = rope_apply(make_float4(kv[0] * rk * wkv[0], kv[1] * rk * wkv[1], kv[2] * rk * wkv[2], kv[3] * rk * wkv[3]), c0, s0);
    const float4 b1 = rope_apply(make_float4(kv[4] * rk * wkv[4], kv[5] * rk * wkv[5], kv[6] * rk * wkv[6], kv[7] * rk * wkv[7]), c1, s1);
    bf16x8 qo, ko;
    qo[0] = (bf16)a0.x; qo[1] = (bf16)a0.y; qo[2] = (bf16)a0.z; qo[3] = (bf16)a0.w; qo[4] = (bf16)a1.x; qo[5] = (bf16)a1.y; qo[6] = (bf16)a1.z; qo[7] = (bf16)a1.w;
    ko[0] = (bf16)b0.x; ko[1] = (bf16)b0.y; ko[2] = (bf16)b0.z; ko[3] = (bf16)b0.w; ko[4] = (bf16)b1.x; ko[5] = (bf16)b1.y; ko[6] = (bf16)b1.z; ko[7] = (bf16)b1.w;
    const size_t dst = ((size_t)(b * H + h) * N + n) * hd + c8;
    __builtin_nontemporal_store(qo, (bf16x8*)(q + dst));
    __builtin_nontemporal_store(ko, (bf16x8*)(k + dst));
  };
  auto src_of = [&](long it) { const int h = it % H; const long bn = it / H; return qkv + ((size_t)bn * 3 * H + h) * hd + c8; };
  long it = gid;
  for (; it + gstride < items; it += 2 * gstride) {          // two items in flight
    const bf16* p0 = src_of(it);
    const bf16* p1 = src_of(it + gstride);
    const bf16x8 q0 = __builtin_nontemporal_load((const bf16x8*)p0), k0 = __builtin_nontemporal_load((const bf16x8*)(p0 + (size_t)H * hd));
    const bf16x8 q1 = __builtin_nontemporal_load((const bf16x8*)p1), k1 = __builtin_nontemporal_load((const bf16x8*)(p1 + (size_t)H * hd));
    one(it, q0, k0);
    one(it + gstride, q1, k1);
  }
  if (it < items) {
    const bf16* p0 = src_of(it);
    one(it, *(const bf16x8*)p0, *(const bf16x8*)(p0 + (size_t)H * hd));
  }
}

// Head dims whose 4-element chunk count is not a power of two (LightningDiT-XL: 72 -> 18 chunks): the lane-group form above rounds the
// group up to 32 lanes and leaves 14 of them idle (2.0 TB/s at hd = 72).  Here the workgroup's threads are packed densely -- thread t
// serves chunk t % cpi of item t / cpi, 14 items x 18 chunks = 252 of 256 threads at hd = 72, consecutive threads on consecutive
// bytes -- and the two row sums go through LDS (every thread adds its item's cpi partials in the same order).  Same arithmetic per element.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_dense_kernel(const T* __restrict__ qkv, const float* __restrict__ wq,
                                                                    const float* __restrict__ wk, const float* __restrict__ cosT,
                                                                    const float* __restrict__ sinT, T* __restrict__ q, T* __restrict__ k,
                                                                    T* __restrict__ v, int B, int N, int H, int hd, float eps) {
  __shared__ float2 red[256];
  const int cpi = hd >> 2, ipw = 256 / cpi, t = threadIdx.x, li = t / cpi, c4 = (t % cpi) * 4;
  const bool lane_ok = li < ipw;
  const long items = (long)B * N * H;
  const float4 wqv = *(const float4*)(wq + c4), wkv = *(const float4*)(wk + c4);
  for (long base = (long)blockIdx.x * ipw; base < items; base += (long)gridDim.x * ipw) {
    const long it = base + li;
    const bool act = lane_ok && it < items;
    // item order: tiles of 8 tokens x H heads, token fastest inside a head -- consecutive items then write consecutive rows of ONE head
    // (8 rows of 144 B = 9 whole lines at hd = 72; with the head fastest every 144-B row is a partial-line write of its own)
    const long tile = it / (8 * H);
    const int rr = (int)(it % (8 * H)), h = rr >> 3;
    const long tok = tile * 8 + (rr & 7);
    const int n = (int)(tok % N), b = (int)(tok / N);
    const T* src = qkv + ((size_t)(b * N + n) * 3 * H + h) * hd + c4;
    const size_t dst = ((size_t)(b * H + h) * N + n) * hd + c4;
    float4 qv = f4(0.f), kv = f4(0.f), vv = f4(0.f), cs = f4(0.f), sn = f4(0.f);
    if (act) {
      qv = load4<T>(src); kv = load4<T>(src + (size_t)H * hd);
      if (v) vv = load4<T>(src + (size_t)2 * H * hd);
      cs = *(const float4*)(cosT + (size_t)n * hd + c4); sn = *(const float4*)(sinT + (size_t)n * hd + c4);
    }
    red[t] = make_float2(hsum(qv * qv), hsum(kv * kv));
    __syncthreads();
    float sq = 0.f, sk = 0.f;
    if (lane_ok) {
      for (int j = 0; j < cpi; ++j) { const float2 p = red[li * cpi + j]; sq += p.x; sk += p.y; }
    }
    __syncthreads();
    if (act) {
      const float rq = rsqrtf(sq / (float)hd + eps), rk = rsqrtf(sk / (float)hd + eps);
      store4<T>(q + dst, rope_apply((qv * rq) * wqv, cs, sn));
      store4<T>(k + dst, rope_apply((kv * rk) * wkv, cs, sn));
      if (v) store4<T>(v + dst, vv);
    }
  }
}

// The bf16 form of the dense kernel with 16-B accesses (8 elements per thread; hd = 72: 9 chunks per item, 28 items x 9 = 252 of 256 threads):
// the 4-element form above moves 8 B per lane -- half-width requests, 3.4 TB/s on the XL/1 forward (4.8 GB per launch at CFG batch 512).
// Same arithmetic and the same association of the row sums (per 4-element chunk, chunks added in order): bitwise the same outputs.
__global__ __launch_bounds__(256) void qknorm_rope_fwd_dense8_kernel(const bf16* __restrict__ qkv, const float* __restrict__ wq,
                                                                     const float* __restrict__ wk, const float* __restrict__ cosT,
                                                                     const float* __restrict__ sinT, bf16* __restrict__ q, bf16* __restrict__ k,
                                                                     bf16* __restrict__ v, int B, int N, int H, int hd, float eps) {
  __shared__ float2 red[512];
  const int cpi = hd >> 3, ipw = 256 / cpi, t = threadIdx.x, li = t / cpi, ci = t % cpi, c8 = ci * 8;
  const bool lane_ok = li < ipw;
  const long items = (long)B * N * H;
  float wqv[8], wkv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { wqv[j] = wq[c8 + j]; wkv[j] = wk[c8 + j]; }
  for (long base = (long)blockIdx.x * ipw; base < items; base += (long)gridDim.x * ipw) {
    const long it = base + li;
    const bool act = lane_ok && it < items;
    const long tile = it / (8 * H);                       // item order as in the 4-element form: 8 tokens x H heads, token fastest inside a head
    const int rr = (int)(it % (8 * H)), h = rr >> 3;
    const long tok = tile * 8 + (rr & 7);
    const int n = (int)(tok % N), b = (int)(tok / N);
    const bf16* src = qkv + ((size_t)(b * N + n) * 3 * H + h) * hd + c8;
    const size_t dst = ((size_t)(b * H + h) * N + n) * hd + c8;
    float qv[8], kv[8];
    bf16x8 vi;
    float4 c0 = f4(0.f), c1 = f4(0.f), s0 = f4(0.f), s1 = f4(0.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) { qv[j] = 0.f; kv[j] = 0.f; }
    if (act) {
      const bf16x8 qi = __builtin_nontemporal_load((const bf16x8*)src), ki = __builtin_nontemporal_load((const bf16x8*)(src + (size_t)H * hd));
      if (v) vi = __builtin_nontemporal_load((const bf16x8*)(src + (size_t)2 * H * hd));
#pragma unroll
      for (int j = 0; j < 8; ++j) { qv[j] = (float)qi[j]; kv[j] = (float)ki[j]; }
      c0 = *(const float4*)(cosT + (size_t)n * hd + c8); c1 = *(const float4*)(cosT + (size_t)n * hd + c8 + 4);
      s0 = *(const float4*)(sinT + (size_t)n * hd + c8); s1 = *(const float4*)(sinT + (size_t)n * hd + c8 + 4);
    }
    red[2 * t] = make_float2((qv[0] * qv[0] + qv[1] * qv[1]) + (qv[2] * qv[2] + qv[3] * qv[3]), (kv[0] * kv[0] + kv[1] * kv[1]) + (kv[2] * kv[2] + kv[3] * kv[3]));
    red[2 * t + 1] = make_float2((qv[4] * qv[4] + qv[5] * qv[5]) + (qv[6] * qv[6] + qv[7] * qv[7]), (kv[4] * kv[4] + kv[5] * kv[5]) + (kv[6] * kv[6] + kv[7] * kv[7]));
    __syncthreads();
    float sq = 0.f, sk = 0.f;
    if (lane_ok) {
      for (int j = 0; j < 2 * cpi; ++j) { const float2 p = red[2 * li * cpi + j]; sq += p.x; sk += p.y; }
    }
    __syncthreads();
    if (act) {
      const float rq = rsqrtf(sq / (float)hd + eps), rk = rsqrtf(sk / (float)hd + eps);
      const float4 a0 = rope_apply(make_float4(qv[0] * rq * wqv[0], qv[1] * rq * wqv[1], qv[2] * rq * wqv[2], qv[3] * rq * wqv[3]), c0, s0);
      const float4 a1 = rope_apply(make_float4(qv[4] * rq * wqv[4], qv[5] * rq * wqv[5], qv[6] * rq * wqv[6], qv[7] * rq * wqv[7]), c1, s1);
      const float4 b0 = rope_apply(make_float4(kv[0] * rk * wkv[0], kv[1] * rk * wkv[1], kv[2] * rk * wkv[2], kv[3] * rk * wkv[3]), c0, s0);
      const float4 b1 = rope_apply(make_float4(kv[4] * rk * wkv[4], kv[5] * rk * wkv[5], kv[6] * rk * wkv[6], kv[7] * rk * wkv[7]), c1, s1);
      bf16x8 qo, ko;
      qo[0] = (bf16)a0.x; qo[1] = (bf16)a0.y; qo[2] = (bf16)a0.z; qo[3] = (bf16)a0.w; qo[4] = (bf16)a1.x; qo[5] = (bf16)a1.y; qo[6] = (bf16)a1.z; qo[7] = (bf16)a1.w;
      ko[0] = (bf16)b0.x; ko[1] = (bf16)b0.y; ko[2] = (bf16)b0.z; ko[3] = (bf16)b0.w; ko[4] = (bf16)b1.x; ko[5] = (bf16)b1.y; ko[6] = (bf16)b1.z; ko[7] = (bf16)b1.w;
      __builtin_nontemporal_store(qo, (bf16x8*)(q + dst));
      __builtin_nontemporal_store(ko, (bf16x8*)(k + dst));
      if (v) __builtin_nontemporal_store(vi, (bf16x8*)(v + dst));
    }
  }
}

template <int LPR, typename T>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const T* __restrict__ dq, const T* __restrict__ dk, const T* __restrict__ dv,
                                                              const T* __restrict__ qkv, const float* __restrict__ wq,
                                                              const float* __restrict__ wk, const float* __restrict__ cosT,
                                                              const float* __restrict__ sinT, T* __restrict__ dqkv, float* __restrict__ P,
                                                              float* __restrict__ Pb, int B, int N, int H, int hd, float eps) {
  // Pb (optional): bias gradient of the qkv Linear = column sums of dqkv AS STORED.  The host makes the group stride a multiple of
  // H, so a lane group keeps one head for all its items and its lanes own fixed columns: three float4 running sums per lane,
  // written as row `gid` of Pb[groups][3*hd] (q | k | v of head gid % H); the host sums the rows of each head.
  __shared__ float4 red[256][2];
  const int sub = threadIdx.x % LPR, c4 = sub * 4;
  const bool act = c4 < hd;
  const long items = (long)B * N * H;
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / LPR, gstride = (long)gridDim.x * 256 / LPR;
  const bool plain = cosT == nullptr;
  const bool norm = wq != nullptr;       // false with tables: RoPE adjoint only (use_qknorm=False); the pre-norm rows are then not read
  const float4 wqv = (act && norm) ? *(const float4*)(wq + c4) : f4(1.f), wkv = (act && norm) ? *(const float4*)(wk + c4) : f4(1.f);
  float4 awq = f4(0.f), awk = f4(0.f), bq = f4(0.f), bk = f4(0.f), bv = f4(0.f);
  auto rnd = [](float4 v) { return make_float4(to_f<T>(from_f<T>(v.x)), to_f<T>(from_f<T>(v.y)), to_f<T>(from_f<T>(v.z)), to_f<T>(from_f<T>(v.w))); };
  for (long it = gid; it < items; it += gstride) {
    const int h = it % H, n = (it / H) % N, b = it / ((long)H * N);
    const size_t so = ((size_t)(b * N + n) * 3 * H + h) * hd + c4;
    const size_t go = ((size_t)(b * H + h) * N + n) * hd + c4;
    if (plain) {
      if (act) {
        const float4 a = load4<T>(dq + go), bb = load4<T>(dk + go), c = load4<T>(dv + go);
        store4<T>(dqkv + so, a);
        store4<T>(dqkv + so + (size_t)H * hd, bb);
        store4<T>(dqkv + so + (size_t)2 * H * hd, c);
        if (Pb) { bq = bq + a; bk = bk + bb; bv = bv + c; }
      }
      continue;
    }
    float4 qv = f4(0.f), kv = f4(0.f), gq = f4(0.f), gk = f4(0.f), gv = f4(0.f), cs = f4(0.f), sn = f4(0.f);
    if (act) {
      if (norm) { qv = load4<T>(qkv + so); kv = load4<T>(qkv + so + (size_t)H * hd); }
      gq = load4<T>(dq + go); gk = load4<T>(dk + go);
      // dv == NULL: the attention backward has already written dv into the v slot of dqkv (ldmae_attention_bwd_pv); it is only
      // read back for the bias-gradient column sums
      if (dv) gv = load4<T>(dv + go); else if (Pb) gv = load4<T>(dqkv + so + (size_t)2 * H * hd);
      cs = *(const float4*)(cosT + (size_t)n * hd + c4); sn = *(const float4*)(sinT + (size_t)n * hd + c4);
    }
    const float rq = norm ? rsqrtf(group_sum<LPR>(hsum(qv * qv)) / (float)hd + eps) : 1.f;      // RoPE only: n = 0, m = 0, r = 1 -> the
    const float rk = norm ? rsqrtf(group_sum<LPR>(hsum(kv * kv)) / (float)hd + eps) : 1.f;      // stored rows are exactly rope^T(g)
    const float4 nq = qv * rq, nk = kv * rk;
    const float4 tq = rope_apply_bwd(gq, cs, sn), tk = rope_apply_bwd(gk, cs, sn);   // grad wrt (n * w)
    awq = awq + tq * nq; awk = awk + tk * nk;
    const float4 dnq = tq * wqv, dnk = tk * wkv;
    const float mq = group_sum<LPR>(hsum(dnq * nq)) / (float)hd, mk = group_sum<LPR>(hsum(dnk * nk)) / (float)hd;
    if (act) {
      const float4 oq = (dnq - nq * mq) * rq, ok = (dnk - nk * mk) * rk;
      store4<T>(dqkv + so, oq);
      store4<T>(dqkv + so + (size_t)H * hd, ok);
      if (dv) store4<T>(dqkv + so + (size_t)2 * H * hd, gv);
      if (Pb) { bq = bq + rnd(oq); bk = bk + rnd(ok); bv = bv + gv; }
    }
  }
  if (Pb && act) {
    float* row = Pb + (size_t)gid * 3 * hd + c4;
    *(float4*)row = bq; *(float4*)(row + hd) = bk; *(float4*)(row + 2 * hd) = bv;
  }
  if (!norm) return;
  red[threadIdx.x][0] = awq; red[threadIdx.x][1] = awk;
  __syncthreads();
  if (threadIdx.x < LPR && act) {
    float4 sq = f4(0.f), sk = f4(0.f);
    for (int t = threadIdx.x; t < 256; t += LPR) { sq = sq + red[t][0]; sk = sk + red[t][1]; }
    *(float4*)(P + (size_t)blockIdx.x * 2 * hd + c4) = sq;
    *(float4*)(P + (size_t)blockIdx.x * 2 * hd + hd + c4) = sk;
  }
}

static unsigned qk_grid(long items, int lpr) {
  long wg = (items * lpr + 255) / 256;
  return (unsigned)(wg < 2048 ? (wg > 0 ? wg : 1) : 2048);
}

extern "C" int ldmae_qknorm_rope_fwd(int dtype, const void* qkv, const float* wq, const float* wk, const float* cos, const float* sin,
                                     void* q, void* k, void* v, int B, int N, int H, int hd, float eps, void* stream) {
  LDMAE_REQUIRE(qkv && q && k && (v || cos), "qknorm_rope_fwd: null pointer (v may be NULL only with RoPE: v then stays in the packed qkv)");
  LDMAE_REQUIRE(!wq == !wk && !cos == !sin && (!wq || cos), "qknorm_rope_fwd: pass wq/wk/cos/sin (QK-norm + RoPE), cos/sin alone (RoPE only: use_qknorm=False), or none (plain head-major relayout)");
  LDMAE_REQUIRE(hd % 8 == 0 && hd <= 128 && B > 0 && N > 0 && H > 0, "qknorm_rope_fwd: head_dim=%d must be a multiple of 8 and <= 128", hd);
  hipStream_t st = as_stream(stream);
  const long items = (long)B * N * H;
  const int cpi = hd / 4;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    auto generic = [&](auto kernel, int lpr) { hipLaunchKernelGGL(kernel, dim3(qk_grid(items, lpr)), dim3(256), 0, st, (const T*)qkv, wq, wk, cos, sin, (T*)q, (T*)k, (T*)v, B, N, H, hd, eps); };
    if (wq && hd > 64 && (cpi & (cpi - 1)) != 0 && N % 8 == 0) {      // e.g. hd = 72: densely packed threads instead of 32-lane groups with 18 busy lanes
      const int per = __is_same(T, bf16) ? hd / 8 : cpi;              // chunks per item: 8 elements (bf16, 16-B accesses) or 4
      const long wgs = (items + 256 / per - 1) / (256 / per);
      const unsigned grid = (unsigned)(wgs < 4096 ? wgs : 4096);
      if constexpr (__is_same(T, bf16)) hipLaunchKernelGGL(qknorm_rope_fwd_dense8_kernel, dim3(grid), dim3(256), 0, st, (const bf16*)qkv, wq, wk, cos, sin, (bf16*)q, (bf16*)k, (bf16*)v, B, N, H, hd, eps);
      else hipLaunchKernelGGL(qknorm_rope_fwd_dense_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)qkv, wq, wk, cos, sin, (T*)q, (T*)k, (T*)v, B, N, H, hd, eps);
      return;
    }
    if constexpr (__is_same(T, bf16)) {
      if (cos && !v && (hd == 64 || hd == 128) && items % (256 / (hd / 8)) == 0) {
        // the LightningDiT block's form (v stays in the packed qkv): 16-B accesses, whole lane groups
        const unsigned grid = qk_grid(items, hd / 8);
        if (hd == 64) hipLaunchKernelGGL(qknorm_rope_fwd8_kernel<8>, dim3(grid), dim3(256), 0, st, (const bf16*)qkv, wq, wk, cos, sin, (bf16*)q, (bf16*)k, B, N, H, eps);
        else hipLaunchKernelGGL(qknorm_rope_fwd8_kernel<16>, dim3(grid), dim3(256), 0, st, (const bf16*)qkv, wq, wk, cos, sin, (bf16*)q, (bf16*)k, B, N, H, eps);
        return;
      }
    }
    if (hd <= 64) generic(qknorm_rope_fwd_kernel<16, T>, 16); else generic(qknorm_rope_fwd_kernel<32, T>, 32);
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "qknorm_rope_fwd: dtype %d (f32 or bf16)", dtype);
  LDMAE_CHECK_LAUNCH("qknorm_rope_fwd");
  return LDMAE_OK;
}

// backward grid: like qk_grid, rounded down so that the lane-group stride (grid * 256 / lpr) is a multiple of H -- every lane group
// then serves ONE head (needed for the fused bias-gradient sums)
static unsigned qk_bwd_grid(long items, int lpr, int H) {
  unsigned g = qk_grid(items, lpr);
  const int gpw = 256 / lpr;
  int a = H, bb = gpw;
  while (bb) { const int t = a % bb; a = bb; bb = t; }       // gcd(H, groups per workgroup)
  const unsigned m = (unsigned)(H / a);
  return g >= m ? g / m * m : m;
}
extern "C" long ldmae_qknorm_rope_bwd_workspace_bytes(int B, int N, int H, int hd) {
  const int lpr = hd <= 64 ? 16 : 32;
  const long grid = qk_bwd_grid((long)B * N * H, lpr, H), groups = grid * (256 / lpr);
  // dwq/dwk partials + bias partial rows [groups][3*hd] + their column-sum scratch
  return grid * 2 * hd * 4 + groups * 3 * hd * 4 + ldmae_colsum_workspace_bytes((int)(groups / H), 3 * H * hd);
}

extern "C" int ldmae_qknorm_rope_bwd(int dtype, const void* dq, const void* dk, const void* dv, const void* qkv, const float* wq,
                                     const float* wk, const float* cos, const float* sin, void* dqkv, float* dwq, float* dwk, float beta_w,
                                     float* dbias_hqd, int B, int N, int H, int hd, float eps, float* workspace, void* stream) {
  LDMAE_REQUIRE(dq && dk && dqkv && (dv || cos), "qknorm_rope_bwd: null pointer (dv may be NULL only with RoPE: dv is then already in dqkv)");
  LDMAE_REQUIRE(!wq == !wk && !cos == !sin && (!wq || (qkv && cos && dwq && dwk)) && (!cos || workspace),
                "qknorm_rope_bwd: pass all norm/rope arguments, cos/sin without wq/wk (RoPE adjoint only: use_qknorm=False), or none of them (plain relayout)");
  LDMAE_REQUIRE(!dbias_hqd || workspace, "qknorm_rope_bwd: dbias requested without workspace");
  LDMAE_REQUIRE(hd % 8 == 0 && hd <= 128 && B > 0 && N > 0 && H > 0, "qknorm_rope_bwd: head_dim=%d must be a multiple of 8 and <= 128", hd);
  hipStream_t st = as_stream(stream);
  const long items = (long)B * N * H;
  const int lpr = hd <= 64 ? 16 : 32;
  const unsigned grid = qk_bwd_grid(items, lpr, H);
  const long groups = (long)grid * (256 / lpr);
  float* Pb = dbias_hqd ? workspace + (size_t)grid * 2 * hd : nullptr;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, (const T*)dq, (const T*)dk, (const T*)dv, (const T*)qkv, wq, wk, cos, sin, (T*)dqkv, workspace, Pb, B, N, H, hd, eps); };
    if (hd <= 64) launch(qknorm_rope_bwd_kernel<16, T>); else launch(qknorm_rope_bwd_kernel<32, T>);
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "qknorm_rope_bwd: dtype %d (f32 or bf16)", dtype);
  LDMAE_CHECK_LAUNCH("qknorm_rope_bwd");
  if (wq) {
    group_reduce(workspace, 2 * hd, 1, hd, grid, dwq, hd, beta_w, st);
    group_reduce(workspace + hd, 2 * hd, 1, hd, grid, dwk, hd, beta_w, st);
    LDMAE_CHECK_LAUNCH("qknorm_rope_bwd reduce");
  }
  // rows g of Pb belong to head g % H: as a [groups/H][H*3*hd] matrix its column sums are the bias gradient in (head, q|k|v, d) order
  if (dbias_hqd) return ldmae_colsum(LDMAE_F32, Pb, 3 * H * hd, (int)(groups / H), 3 * H * hd, dbias_hqd, 0.f, Pb + (size_t)groups * 3 * hd, stream);
  return LDMAE_OK;
}

// ------------------------------------------------------------------ standalone RoPE (VisionRotaryEmbeddingFast.forward, pos_embed.py:135)
// out[r, :] = t[r, :] * cos[r % N, :] + rotate_half(t[r, :]) * sin[r % N, :]  (rotate_half: (x0, x1) -> (-x1, x0) per pair);
// transposed = 1: the adjoint (its backward).  The block path never comes here (RoPE is fused into ldmae_qknorm_rope_*).
template <typename T>
__global__ void rope_kernel(const T* __restrict__ t, const float* __restrict__ cosT, const float* __restrict__ sinT, T* __restrict__ out,
                            long rows, int N, int hd, int transposed) {
  const long n4 = rows * (hd / 4), per = hd / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const long r = i / per;
    const int c4 = (int)(i % per) * 4, n = (int)(r % N);
    const float4 v = load4<T>(t + r * hd + c4);
    const float4 cs = *(const float4*)(cosT + (size_t)n * hd + c4), sn = *(const float4*)(sinT + (size_t)n * hd + c4);
    store4<T>(out + r * hd + c4, transposed ? rope_apply_bwd(v, cs, sn) : rope_apply(v, cs, sn));
  }
}

extern "C" int ldmae_rope(int dtype, const void* t, const float* cos, const float* sin, void* out, long rows, int N, int hd, int transposed,
                          void* stream) {
  LDMAE_REQUIRE(t && cos && sin && out && rows > 0 && N > 0, "rope: null pointer or empty input");
  LDMAE_REQUIRE(hd % 4 == 0 && rows % N == 0, "rope: head_dim=%d must be a multiple of 4 and rows=%ld a multiple of N=%d", hd, rows, N);
  const long n4 = rows * (hd / 4);
  const unsigned grid = (unsigned)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  auto go = [&](auto tt) { using T = tag_t<decltype(tt)>; hipLaunchKernelGGL(rope_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T*)t, cos, sin, (T*)out, rows, N, hd, transposed); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "rope: bad dtype %d", dtype);
  LDMAE_CHECK_LAUNCH("rope");
  return LDMAE_OK;
}
