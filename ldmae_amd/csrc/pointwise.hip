// Pointwise / streaming kernels around the LightningDiT block (gfx950, wave64): SwiGLU, column sums, casts, thin GEMMs, multi_add, embedders, AdamW + EMA.
#include "rowwise_common.h"

// ------------------------------------------------------------------ SwiGLU
template <typename T>
__global__ void swiglu_fwd_kernel(const T* __restrict__ h12, T* __restrict__ hid, long M, int Hs) {
  const long n8 = M * Hs / 8, per_row = Hs / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long m = i / per_row, c = (i % per_row) * 8;
    float a[8], b[8], o[8];
    Vec8<T>::load(h12 + m * 2 * Hs + c, a);
    Vec8<T>::load(h12 + m * 2 * Hs + Hs + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = a[j] * fast_sigmoid(a[j]) * b[j];
    Vec8<T>::store(hid + m * Hs + c, o);
  }
}
template <typename T>
__global__ void swiglu_bwd_kernel(const T* __restrict__ dhid, const T* __restrict__ h12, T* __restrict__ dh12, long M, int Hs) {
  const long n8 = M * Hs / 8, per_row = Hs / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long m = i / per_row, c = (i % per_row) * 8;
    float a[8], b[8], g[8], da[8], db[8];
    Vec8<T>::load(h12 + m * 2 * Hs + c, a);
    Vec8<T>::load(h12 + m * 2 * Hs + Hs + c, b);
    Vec8<T>::load(dhid + m * Hs + c, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = fast_sigmoid(a[j]);
      da[j] = g[j] * b[j] * s * (1.f + a[j] * (1.f - s));
      db[j] = g[j] * a[j] * s;
    }
    Vec8<T>::store(dh12 + m * 2 * Hs + c, da);
    Vec8<T>::store(dh12 + m * 2 * Hs + Hs + c, db);
  }
}

extern "C" int ldmae_swiglu_fwd(int dtype, const void* h12, void* hid, int M, int Hs, void* stream) {
  LDMAE_REQUIRE(h12 && hid && M > 0 && Hs > 0 && Hs % 8 == 0, "swiglu_fwd: bad arguments (Hs=%d must be a multiple of 8)", Hs);
  const unsigned grid = ew_grid((long)M * Hs / 8);
  auto go = [&](auto t) { using T = tag_t<decltype(t)>; hipLaunchKernelGGL(swiglu_fwd_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T*)h12, (T*)hid, (long)M, Hs); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "swiglu_fwd: dtype %d (f32 or bf16)", dtype);
  LDMAE_CHECK_LAUNCH("swiglu_fwd");
  return LDMAE_OK;
}
extern "C" int ldmae_swiglu_bwd(int dtype, const void* dhid, const void* h12, void* dh12, int M, int Hs, void* stream) {
  LDMAE_REQUIRE(dhid && h12 && dh12 && M > 0 && Hs > 0 && Hs % 8 == 0, "swiglu_bwd: bad arguments (Hs=%d must be a multiple of 8)", Hs);
  const unsigned grid = ew_grid((long)M * Hs / 8);
  auto go = [&](auto t) { using T = tag_t<decltype(t)>; hipLaunchKernelGGL(swiglu_bwd_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T*)dhid, (const T*)h12, (T*)dh12, (long)M, Hs); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dtype, go)), "swiglu_bwd: dtype %d (f32 or bf16)", dtype);
  LDMAE_CHECK_LAUNCH("swiglu_bwd");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ column sums (bias gradients)
// rows summed by one workgroup: enough row groups for ~512 workgroups (the adaLN bias gradient is 256 rows x 4608 columns:
// with a fixed 256 rows it ran on 5 workgroups, 65 us for 4.7 MB)
static int colsum_rows(int M, int N) {
  const long colblocks = cdiv(N, 1024);
  long groups = 512 / colblocks; if (groups < 1) groups = 1;
  long rows = (M + groups - 1) / groups;
  int r = 8; while (r < rows && r < 256) r <<= 1;
  return r;
}
// a column block narrower than 1024 columns leaves threads without a column: they take interleaved rows of the same columns instead
// (N = 128: 8 row streams per workgroup instead of 32 busy threads) and the streams are summed in fixed order through LDS
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ X, int ldx, int M, int N, int rows, float* __restrict__ P) {
  __shared__ float4 red[256];
  const int ncol4 = min(N / 4 - (int)blockIdx.x * 256, 256), nsub = 256 / ncol4;
  const int ci = threadIdx.x % ncol4, rsub = threadIdx.x / ncol4, c = (blockIdx.x * 256 + ci) * 4;
  const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
  float4 s = f4(0.f);
  if (rsub < nsub)
    for (int m = m0 + rsub; m < m1; m += nsub) s = s + load4<T>(X + (size_t)m * ldx + c);
  if (nsub > 1) {
    red[threadIdx.x] = s;
    __syncthreads();
    if (rsub == 0)
      for (int k = 1; k < nsub; ++k) s = s + red[k * ncol4 + ci];
  }
  if (rsub == 0) *(float4*)(P + (size_t)blockIdx.y * N + c) = s;
}
extern "C" long ldmae_colsum_workspace_bytes(int M, int N) { return (long)cdiv(M, colsum_rows(M, N)) * N * 4; }
extern "C" int ldmae_colsum(int dtype, const void* X, int ldx, int M, int N, float* out, float beta, float* workspace, void* stream) {
  LDMAE_REQUIRE(X && out && workspace && M > 0 && N > 0 && N % 4 == 0 && ldx % 4 == 0, "colsum: bad arguments (N=%d ldx=%d multiples of 4)", N, ldx);
  hipStream_t st = as_stream(stream);
  const int rows = colsum_rows(M, N), G = cdiv(M, rows);
  auto go = [&](auto t) { using T = tag_t<decltype(t)>; hipLaunchKernelGGL(colsum_kernel<T>, dim3(cdiv(N, 1024), G), dim3(256), 0, st, (const T*)X, ldx, M, N, rows, workspace); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16, f16>(dtype, go)), "colsum: dtype %d (f32, bf16 or f16)", dtype);
  group_reduce(workspace, N, 1, N, G, out, N, beta, st);
  LDMAE_CHECK_LAUNCH("colsum");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ casts
template <typename S, typename Dt>
__global__ void cast_kernel(const S* __restrict__ s, Dt* __restrict__ d, long n) {
  const long n8 = n / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    Vec8<S>::load(s + i * 8, v);
    Vec8<Dt>::store(d + i * 8, v);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) d[n8 * 8 + threadIdx.x] = from_f<Dt>(to_f<S>(s[n8 * 8 + threadIdx.x]));
}
extern "C" int ldmae_cast(int src_dtype, int dst_dtype, const void* src, void* dst, long n, void* stream) {
  LDMAE_REQUIRE(src && dst && n > 0, "cast: null pointer or empty");
  LDMAE_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "cast: pointers must be 16-B aligned");
  hipStream_t st = as_stream(stream);
  const unsigned grid = ew_grid(n / 8 + 1);
  bool ok = false;
  dtype_dispatch<float, bf16, f16>(src_dtype, [&](auto s) {
    using S = tag_t<decltype(s)>;
    auto to = [&](auto d) { using Dt = tag_t<decltype(d)>; hipLaunchKernelGGL((cast_kernel<S, Dt>), dim3(grid), dim3(256), 0, st, (const S*)src, (Dt*)dst, n); };
    if constexpr (__is_same(S, float)) ok = dtype_dispatch<float, bf16, f16>(dst_dtype, to);
    else ok = dtype_dispatch<float>(dst_dtype, to);                  // a 16-bit source widens to f32 only
  });
  LDMAE_REQUIRE(ok, "cast: unsupported %d -> %d", src_dtype, dst_dtype);
  LDMAE_CHECK_LAUNCH("cast");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ thin GEMMs: contraction length K <= 32 over M = batch * tokens rows
// The DiT's PatchEmbed at patch 1 (lightningdit.py:309, 402: K = C * p * p = 16) and the dX of the FinalLayer's 16-column Linear (:270)
// are [M, 768] <-> [M, 16] products at M = 262144: 0.02 FLOP per byte, pure HBM streaming.  As 64x64-tile MFMA GEMMs they ran at
// 2.2 TB/s (358 us forward, 366 + 34 + 146 us for weight gradient + split reduce + bias column sum: two passes over the 805-MB
// gradient).  Here the K-vectors of a workgroup's rows sit in LDS (broadcast reads) and the weights / partial sums live in registers: one
// pass over the big tensor.
//   thin_nt: out[m, n] = sum_k T[m, k] W[n, k] + bias[n] (+ pos[m % rows_per_batch, n])
//   thin_tn: dW[n, k] = sum_m G[m, n] T[m, k], dbias[n] = sum_m G[m, n]   (per-chunk partials, summed in fixed order by splitk_reduce)
template <int K, typename OutT, bool POS>
__global__ __launch_bounds__(256) void thin_nt_kernel(const float* __restrict__ T, const float* __restrict__ W, const float* __restrict__ bias,
                                                      const float* __restrict__ pos, OutT* __restrict__ out, int M, int N, int rows_per_batch,
                                                      int rows_per_wg) {
  // the workgroup's rows of T (128 x K floats) are staged in LDS once (coalesced 16-B loads) and read back at a wave-uniform address
  // (LDS broadcast); a thread owns FOUR adjacent columns, so a wave stores whole 1-KiB runs (one column per thread moved 4 B per lane:
  // 2.5 TB/s); 128 rows per workgroup keep ~6 waves per SIMD in flight
  __shared__ __attribute__((aligned(16))) float ts[128 * K];
  const int m0 = blockIdx.x * rows_per_wg, m1 = min(M, m0 + rows_per_wg);
  for (int i = threadIdx.x * 4; i < (m1 - m0) * K; i += 256 * 4) *(float4*)(ts + i) = *(const float4*)(T + (size_t)m0 * K + i);
  __syncthreads();
  const int n = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (n >= N) return;
  float w[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; k += 4) {
      const float4 v = *(const float4*)(W + (size_t)(n + j) * K + k);
      w[j][k] = v.x; w[j][k + 1] = v.y; w[j][k + 2] = v.z; w[j][k + 3] = v.w;
    }
  const float4 b = bias ? *(const float4*)(bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
  for (int m = m0; m < m1; ++m) {
    const float* t = ts + (m - m0) * K;
    float a0 = b.x, a1 = b.y, a2 = b.z, a3 = b.w;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float tk = t[k];
      a0 = fmaf(tk, w[0][k], a0); a1 = fmaf(tk, w[1][k], a1); a2 = fmaf(tk, w[2][k], a2); a3 = fmaf(tk, w[3][k], a3);
    }
    if (POS) {
      const float4 q = *(const float4*)(pos + (size_t)(m % rows_per_batch) * N + n);
      a0 += q.x; a1 += q.y; a2 += q.z; a3 += q.w;
    }
    if constexpr (sizeof(OutT) == 4) *(float4*)((float*)out + (size_t)m * N + n) = make_float4(a0, a1, a2, a3);
    else { bf16x4 o; o[0] = (bf16)a0; o[1] = (bf16)a1; o[2] = (bf16)a2; o[3] = (bf16)a3; *(bf16x4*)((bf16*)out + (size_t)m * N + n) = o; }
  }
}

template <int K>
__global__ __launch_bounds__(256) void thin_tn_kernel(const float* __restrict__ G, const float* __restrict__ T, float* __restrict__ P,
                                                      float* __restrict__ Pb, int M, int N, int rows_per_wg) {
  __shared__ __attribute__((aligned(16))) float ts[512 * K];
  const int m0 = blockIdx.x * rows_per_wg, m1 = min(M, m0 + rows_per_wg);
  for (int i = threadIdx.x * 4; i < (m1 - m0) * K; i += 256 * 4) *(float4*)(ts + i) = *(const float4*)(T + (size_t)m0 * K + i);
  __syncthreads();
  const int n = blockIdx.y * 256 + threadIdx.x;
  if (n >= N) return;
  float acc[K], accb = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll 4
  for (int m = m0; m < m1; ++m) {
    const float g = G[(size_t)m * N + n];
    const float* t = ts + (m - m0) * K;                 // wave-uniform LDS address: broadcast reads
    accb += g;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = fmaf(g, t[k], acc[k]);
  }
  float* p = P + ((size_t)blockIdx.x * N + n) * K;
#pragma unroll
  for (int k = 0; k < K; k += 4) *(float4*)(p + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
  if (Pb) Pb[(size_t)blockIdx.x * N + n] = accb;
}
// out[i] = beta * out[i] + sum_c P[c][i], i < n, in a FIXED order (deterministic): one wave per 4 consecutive outputs, lane l sums chunks
// l, l + 64, ... and the 64 lane sums are folded by a butterfly -- few outputs (12288) x many chunks (512) needs its parallelism across chunks
__global__ __launch_bounds__(256) void thin_reduce_kernel(const float* __restrict__ P, float* __restrict__ out, long n, int chunks, float beta) {
  const int lane = threadIdx.x & 63;
  const long i = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (i >= n) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = lane; c < chunks; c += 64) {
    const float4 t = *(const float4*)(P + (size_t)c * n + i);
    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s.x += __shfl_xor(s.x, o, 64); s.y += __shfl_xor(s.y, o, 64); s.z += __shfl_xor(s.z, o, 64); s.w += __shfl_xor(s.w, o, 64);
  }
  if (lane == 0) {
    if (beta != 0.f) { const float4 o = *(const float4*)(out + i); s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w; }
    *(float4*)(out + i) = s;
  }
}
constexpr int THIN_ROWS = 512;      // rows of M per workgroup (the kernels' LDS image of T is sized for it)
static bool thin_ok(int N, int K) { return (K == 16 || K == 32) && N % 4 == 0 && N >= 4; }

extern "C" int ldmae_thin_nt(int out_dtype, const float* T, const float* W, const float* bias, const float* pos, void* out, int M, int N, int K,
                             int rows_per_batch, void* stream) {
  LDMAE_REQUIRE(T && W && out && M > 0, "thin_nt: null pointer or empty input");
  LDMAE_REQUIRE(thin_ok(N, K), "thin_nt: K=%d must be 16 or 32 and N=%d a multiple of 4 (use ldmae_gemm_nt otherwise)", K, N);
  LDMAE_REQUIRE(!pos || rows_per_batch > 0, "thin_nt: pos needs rows_per_batch");
  const dim3 grid(cdiv(M, 128), cdiv(N / 4, 256));
  hipStream_t st = as_stream(stream);
  auto go = [&](auto t) {
    using OT = tag_t<decltype(t)>;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, T, W, bias, pos, (OT*)out, M, N, rows_per_batch, 128); };
    if (K == 16) { if (pos) launch(thin_nt_kernel<16, OT, true>); else launch(thin_nt_kernel<16, OT, false>); }
    else { if (pos) launch(thin_nt_kernel<32, OT, true>); else launch(thin_nt_kernel<32, OT, false>); }
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(out_dtype, go)), "thin_nt: bad out dtype %d", out_dtype);
  LDMAE_CHECK_LAUNCH("thin_nt");
  return LDMAE_OK;
}
extern "C" long ldmae_thin_tn_workspace_bytes(int M, int N, int K) { return (long)cdiv(M, THIN_ROWS) * ((long)N * K + N) * 4; }
extern "C" int ldmae_thin_tn(const float* G, const float* T, float* dW, float* dbias, int M, int N, int K, float beta, float* workspace,
                             long workspace_bytes, void* stream) {
  LDMAE_REQUIRE(G && T && dW && M > 0, "thin_tn: null pointer or empty input");
  LDMAE_REQUIRE(thin_ok(N, K), "thin_tn: K=%d must be 16 or 32 and N=%d a multiple of 4 (use ldmae_gemm_tn otherwise)", K, N);
  LDMAE_REQUIRE(beta == 0.f || beta == 1.f, "thin_tn: beta must be 0 or 1");
  LDMAE_REQUIRE(workspace && workspace_bytes >= ldmae_thin_tn_workspace_bytes(M, N, K), "thin_tn: workspace too small");
  const int chunks = cdiv(M, THIN_ROWS);
  float* P = workspace;
  float* Pb = dbias ? workspace + (size_t)chunks * N * K : nullptr;
  const dim3 grid(chunks, cdiv(N, 256));
  hipStream_t st = as_stream(stream);
  if (K == 16) hipLaunchKernelGGL(thin_tn_kernel<16>, grid, dim3(256), 0, st, G, T, P, Pb, M, N, THIN_ROWS);
  else hipLaunchKernelGGL(thin_tn_kernel<32>, grid, dim3(256), 0, st, G, T, P, Pb, M, N, THIN_ROWS);
  const long n = (long)N * K;
  hipLaunchKernelGGL(thin_reduce_kernel, dim3((unsigned)((n / 4 + 3) / 4)), dim3(256), 0, st, P, dW, n, chunks, beta);
  if (dbias) hipLaunchKernelGGL(thin_reduce_kernel, dim3(cdiv(N / 4, 4)), dim3(256), 0, st, Pb, dbias, (long)N, chunks, beta);
  LDMAE_CHECK_LAUNCH("thin_tn");
  return LDMAE_OK;
}

// dst[i] += src[i] for up to 32 (dst, src, n) f32 triples in ONE launch: the small parameter gradients of a block (norm weights, biases, QK-norm
// weights) added into their .grad views of the optimizer's slab -- as separate AccumulateGrad adds they were 8 launches of ~5 us per block.
constexpr int MULTI_ADD_MAX = 32;
struct MultiAddArgs { float* dst[MULTI_ADD_MAX]; const float* src[MULTI_ADD_MAX]; long n[MULTI_ADD_MAX]; };
__global__ void multi_add_kernel(MultiAddArgs a) {
  float* d = a.dst[blockIdx.y];
  const float* s = a.src[blockIdx.y];
  const long n = a.n[blockIdx.y];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) d[i] += s[i];
}
extern "C" int ldmae_multi_add(int count, void* const* dst, const void* const* src, const long* n, void* stream) {
  LDMAE_REQUIRE(dst && src && n && count > 0 && count <= MULTI_ADD_MAX, "multi_add: count=%d must be 1..%d", count, MULTI_ADD_MAX);
  MultiAddArgs a{};
  long nmax = 0;
  for (int i = 0; i < count; ++i) {
    LDMAE_REQUIRE(dst[i] && src[i] && n[i] > 0, "multi_add: entry %d is null or empty", i);
    a.dst[i] = (float*)dst[i]; a.src[i] = (const float*)src[i]; a.n[i] = n[i];
    nmax = n[i] > nmax ? n[i] : nmax;
  }
  const unsigned gx = (unsigned)min((long)256, (nmax + 255) / 256);
  hipLaunchKernelGGL(multi_add_kernel, dim3(gx, count), dim3(256), 0, as_stream(stream), a);
  LDMAE_CHECK_LAUNCH("multi_add");
  return LDMAE_OK;
}

// `count` equally sized f32 tensors -> one stacked tensor in the activation type with ONE launch (the adaLN weights of all blocks become the
// [depth * 6D, D] operand of a single GEMM: models/lightningdit.py:_AdaLNAllFn).  The source pointers travel by value in the kernel arguments.
constexpr int CAST_STACK_MAX = 64;
struct CastStackArgs { const float* src[CAST_STACK_MAX]; };
template <typename Dt>
__global__ void cast_stack_kernel(CastStackArgs a, Dt* __restrict__ dst, long n_each) {
  const float* s = a.src[blockIdx.y];
  Dt* d = dst + (size_t)blockIdx.y * n_each;
  const long n8 = n_each / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    Vec8<float>::load(s + i * 8, v);
    Vec8<Dt>::store(d + i * 8, v);
  }
}
extern "C" int ldmae_cast_stack(int dst_dtype, const void* const* srcs, int count, long n_each, void* dst, void* stream) {
  LDMAE_REQUIRE(srcs && dst && count > 0 && count <= CAST_STACK_MAX, "cast_stack: count=%d must be 1..%d", count, CAST_STACK_MAX);
  LDMAE_REQUIRE(n_each > 0 && n_each % 8 == 0, "cast_stack: n_each=%ld must be a positive multiple of 8", n_each);
  LDMAE_REQUIRE(((uintptr_t)dst & 15) == 0, "cast_stack: dst must be 16-B aligned");
  CastStackArgs a{};
  for (int i = 0; i < count; ++i) {
    LDMAE_REQUIRE(srcs[i] && ((uintptr_t)srcs[i] & 15) == 0, "cast_stack: source %d is null or not 16-B aligned", i);
    a.src[i] = (const float*)srcs[i];
  }
  const unsigned gx = (unsigned)min((long)1024, (n_each / 8 + 255) / 256);
  auto go = [&](auto t) { using Dt = tag_t<decltype(t)>; hipLaunchKernelGGL(cast_stack_kernel<Dt>, dim3(gx, count), dim3(256), 0, as_stream(stream), a, (Dt*)dst, n_each); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(dst_dtype, go)), "cast_stack: unsupported dst dtype %d", dst_dtype);
  LDMAE_CHECK_LAUNCH("cast_stack");
  return LDMAE_OK;
}

// f32 [R,C] -> T [R,C] and T [C,R] through a 32x33 LDS tile
template <typename T>
__global__ __launch_bounds__(256) void cast_weight_kernel(const float* __restrict__ src, T* __restrict__ dst, T* __restrict__ dstT, int R, int C) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    float v = 0.f;
    if (r < R && c < C) { v = src[(size_t)r * C + c]; if (dst) dst[(size_t)r * C + c] = from_f<T>(v); }
    tile[j][tx] = v;
  }
  __syncthreads();
  if (!dstT) return;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (r < R && c < C) dstT[(size_t)c * R + r] = from_f<T>(tile[tx][j]);
  }
}
// The same for shapes whose sides are multiples of 64 (every Linear weight of the shipped models): 64x64 tiles, 16-B loads, 8-B stores of the
// straight copy and 32-B runs of the transposed one (the 4-byte-per-lane form above ran at ~2 TB/s: 48 launches = 0.34 ms per train step)
template <typename T>
__global__ __launch_bounds__(256) void cast_weight64_kernel(const float* __restrict__ src, T* __restrict__ dst, T* __restrict__ dstT, int R, int C) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int lr = threadIdx.x >> 4, lc = (threadIdx.x & 15) * 4;          // 16 rows x 16 float4 per pass
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = p * 16 + lr;
    const float4 v = *(const float4*)(src + (size_t)(r0 + r) * C + c0 + lc);
    if (dst) {
      T* d = dst + (size_t)(r0 + r) * C + c0 + lc;
      if constexpr (sizeof(T) == 4) *(float4*)d = v;
      else { typename Pack<T>::v4 o; o[0] = from_f<T>(v.x); o[1] = from_f<T>(v.y); o[2] = from_f<T>(v.z); o[3] = from_f<T>(v.w); *(typename Pack<T>::v4*)d = o; }
    }
    tile[r][lc] = v.x; tile[r][lc + 1] = v.y; tile[r][lc + 2] = v.z; tile[r][lc + 3] = v.w;
  }
  __syncthreads();
  if (!dstT) return;
  const int c = threadIdx.x >> 2, rq = (threadIdx.x & 3) * 16;            // output row c of the transposed tile, 16 of its 64 values
  T* d = dstT + (size_t)(c0 + c) * R + r0 + rq;
#pragma unroll
  for (int k = 0; k < 16; k += 4) {
    const float a0 = tile[rq + k][c], a1 = tile[rq + k + 1][c], a2 = tile[rq + k + 2][c], a3 = tile[rq + k + 3][c];
    if constexpr (sizeof(T) == 4) *(float4*)(d + k) = make_float4(a0, a1, a2, a3);
    else { typename Pack<T>::v4 o; o[0] = from_f<T>(a0); o[1] = from_f<T>(a1); o[2] = from_f<T>(a2); o[3] = from_f<T>(a3); *(typename Pack<T>::v4*)(d + k) = o; }
  }
}
extern "C" int ldmae_cast_weight(int dst_dtype, const float* src, void* dst, void* dstT, int R, int C, void* stream) {
  LDMAE_REQUIRE(src && (dst || dstT) && R > 0 && C > 0, "cast_weight: null pointer or empty");
  const bool al = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)dstT & 15) == 0;
  auto go = [&](auto t) {
    using T = tag_t<decltype(t)>;
    if (R % 64 == 0 && C % 64 == 0 && al) hipLaunchKernelGGL(cast_weight64_kernel<T>, dim3(C / 64, R / 64), dim3(256), 0, as_stream(stream), src, (T*)dst, (T*)dstT, R, C);
    else hipLaunchKernelGGL(cast_weight_kernel<T>, dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), 0, as_stream(stream), src, (T*)dst, (T*)dstT, R, C);
  };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16, f16>(dst_dtype, go)), "cast_weight: dtype %d (f32, bf16 or f16)", dst_dtype);
  LDMAE_CHECK_LAUNCH("cast_weight");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ embedders
__global__ void timestep_embedding_kernel(const float* __restrict__ t, float* __restrict__ out, int B, int dim, float max_period) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, j = i % half;
  // lightningdit.py:124-129: freqs = exp(-log(max_period) * j / half); args = t * freqs; [cos | sin]
  const float freq = expf(-logf(max_period) * (float)j / (float)half);
  const float a = t[b] * freq;
  out[(size_t)b * dim + j] = cosf(a);
  out[(size_t)b * dim + half + j] = sinf(a);
  if ((dim & 1) && j == 0) out[(size_t)b * dim + dim - 1] = 0.f;
}
extern "C" int ldmae_timestep_embedding(const float* t, float* out, int B, int dim, float max_period, void* stream) {
  LDMAE_REQUIRE(t && out && B > 0 && dim >= 2, "timestep_embedding: bad arguments");
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv((long)B * (dim / 2), 256)), dim3(256), 0, as_stream(stream), t, out, B, dim, max_period);
  LDMAE_CHECK_LAUNCH("timestep_embedding");
  return LDMAE_OK;
}

template <typename OutT>
__global__ void silu_fwd_kernel(const float* __restrict__ x, OutT* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    out[i] = from_f<OutT>(v / (1.f + expf(-v)));
  }
}
__global__ void silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i], s = 1.f / (1.f + expf(-v));
    dx[i] = dy[i] * s * (1.f + v * (1.f - s));
  }
}
extern "C" int ldmae_silu_fwd(int out_dtype, const float* x, void* out, long n, void* stream) {
  LDMAE_REQUIRE(x && out && n > 0, "silu_fwd: bad arguments");
  auto go = [&](auto t) { using T = tag_t<decltype(t)>; hipLaunchKernelGGL(silu_fwd_kernel<T>, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), x, (T*)out, n); };
  LDMAE_REQUIRE((dtype_dispatch<float, bf16>(out_dtype, go)), "silu_fwd: dtype %d (f32 or bf16)", out_dtype);
  LDMAE_CHECK_LAUNCH("silu_fwd");
  return LDMAE_OK;
}
extern "C" int ldmae_silu_bwd(const float* dy, const float* x, float* dx, long n, void* stream) {
  LDMAE_REQUIRE(dy && x && dx && n > 0, "silu_bwd: bad arguments");
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), dy, x, dx, n);
  LDMAE_CHECK_LAUNCH("silu_bwd");
  return LDMAE_OK;
}

__global__ void label_embed_fwd_kernel(const float* __restrict__ table, const long long* __restrict__ y, const unsigned char* __restrict__ drop,
                                       float* __restrict__ out, int B, int D, int num_classes) {
  const int b = blockIdx.x;
  const long long row = (drop && drop[b]) ? num_classes : y[b];
  for (int d = threadIdx.x; d < D; d += blockDim.x) out[(size_t)b * D + d] = table[(size_t)row * D + d];
}
__global__ void label_embed_bwd_kernel(const float* __restrict__ dout, const long long* __restrict__ y, const unsigned char* __restrict__ drop,
                                       float* __restrict__ dtable, int B, int D, int num_classes) {
  // one workgroup per table row; the samples that hit the row are found cooperatively (one sample per thread and pass: a ballot per wave) and
  // summed in ascending sample order (deterministic) by walking the set bits.  (Every thread used to scan all B labels itself: 140 us for a
  // 3 MB result; then a 256-step loop over a hit array in LDS: 84 us.)
  __shared__ unsigned long long mask[4];
  const int row = blockIdx.x, wave = threadIdx.x >> 6;
  for (int b0 = 0; b0 < B; b0 += blockDim.x) {
    const int b = b0 + threadIdx.x;
    const bool mine = b < B && ((drop && drop[b]) ? num_classes : y[b]) == row;
    const unsigned long long m = __ballot(mine);
    if ((threadIdx.x & 63) == 0) mask[wave] = m;
    __syncthreads();
    if ((mask[0] | mask[1] | mask[2] | mask[3]) != 0ull) {
      for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int w = 0; w < 4; ++w)
          for (unsigned long long mm = mask[w]; mm; mm &= mm - 1) s += dout[(size_t)(b0 + w * 64 + __builtin_ctzll(mm)) * D + d];
        dtable[(size_t)row * D + d] += s;
      }
    }
    __syncthreads();
  }
}
extern "C" int ldmae_label_embed_fwd(const float* table, const long long* y, const unsigned char* drop, float* out, int B, int D,
                                     int num_classes, void* stream) {
  LDMAE_REQUIRE(table && y && out && B > 0 && D > 0, "label_embed_fwd: bad arguments");
  hipLaunchKernelGGL(label_embed_fwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), table, y, drop, out, B, D, num_classes);
  LDMAE_CHECK_LAUNCH("label_embed_fwd");
  return LDMAE_OK;
}
extern "C" int ldmae_label_embed_bwd(const float* dout, const long long* y, const unsigned char* drop, float* dtable, int B, int D,
                                     int num_classes, int rows, void* stream) {
  LDMAE_REQUIRE(dout && y && dtable && B > 0 && D > 0 && rows > 0, "label_embed_bwd: bad arguments");
  hipLaunchKernelGGL(label_embed_bwd_kernel, dim3(rows), dim3(256), 0, as_stream(stream), dout, y, drop, dtable, B, D, num_classes);
  LDMAE_CHECK_LAUNCH("label_embed_bwd");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ fused AdamW + EMA over flat f32 buffers
// Scalars are prepared on the host exactly as torch does (python doubles rounded to f32 at the point of use):
// torch/optim/adamw.py _single_tensor_adamw (train_accum.py:121) then ema.mul_(d).add_(p, alpha=1-d) (:336-347).
struct AdamArgs { float decay_mul, w1, beta2, w2, bc2_sqrt, eps, neg_step, ema_d, ema_a, gscale; };
__global__ void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 float* __restrict__ ema, long n, AdamArgs a) {
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    float4 pv = *(float4*)(p + i), gv = *(const float4*)(g + i), mv = *(float4*)(m + i), vv = *(float4*)(v + i);
    float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
    float ea[4] = {0, 0, 0, 0};
    if (ema) { float4 e = *(float4*)(ema + i); ea[0] = e.x; ea[1] = e.y; ea[2] = e.z; ea[3] = e.w; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = a.gscale == 1.f ? ga[j] : ga[j] * a.gscale;
      pa[j] = pa[j] * a.decay_mul;                                  // p.mul_(1 - lr*wd)
      ma[j] = ma[j] + a.w1 * (gj - ma[j]);                          // exp_avg.lerp_(grad, 1-beta1)
      va[j] = va[j] * a.beta2 + a.w2 * (gj * gj);                   // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
      const float denom = sqrtf(va[j]) / a.bc2_sqrt + a.eps;        // (sqrt(v)/bc2_sqrt).add_(eps)
      pa[j] = pa[j] + a.neg_step * (ma[j] / denom);                 // p.addcdiv_(m, denom, value=-step_size)
      ea[j] = ea[j] * a.ema_d + a.ema_a * pa[j];
    }
    *(float4*)(p + i) = make_float4(pa[0], pa[1], pa[2], pa[3]);
    *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
    *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
    if (ema) *(float4*)(ema + i) = make_float4(ea[0], ea[1], ea[2], ea[3]);
  }
}
extern "C" int ldmae_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long n, int step, double lr, double beta1,
                               double beta2, double eps, double weight_decay, double ema_decay, double grad_scale, void* stream) {
  LDMAE_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw_ema: bad arguments");
  LDMAE_REQUIRE(n % 4 == 0, "adamw_ema: flat length %ld must be padded to a multiple of 4", n);
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  AdamArgs a;
  a.decay_mul = (float)(1.0 - lr * weight_decay);
  a.w1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.w2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)eps;
  a.neg_step = (float)(-(lr / bc1));
  a.ema_d = (float)ema_decay;
  a.ema_a = (float)(1.0 - ema_decay);
  a.gscale = (float)grad_scale;
  hipLaunchKernelGGL(adamw_ema_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), p, g, m, v, ema, n, a);
  LDMAE_CHECK_LAUNCH("adamw_ema");
  return LDMAE_OK;
}
__global__ void ema_only_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float d, float a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) ema[i] = ema[i] * d + a * p[i];
}
extern "C" int ldmae_ema_only(float* ema, const float* p, long n, double ema_decay, void* stream) {
  LDMAE_REQUIRE(ema && p && n > 0, "ema_only: bad arguments");
  hipLaunchKernelGGL(ema_only_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), ema, p, n, (float)ema_decay, (float)(1.0 - ema_decay));
  LDMAE_CHECK_LAUNCH("ema_only");
  return LDMAE_OK;
}

// ------------------------------------------------------------------ AdamW + EMA + power-function EMA tracks (post-hoc EMA)
// Karras et al. 2024 ("Analyzing and Improving the Training Dynamics of Diffusion Models", section 3).  Step t counts optimizer steps from 1;
// with exponent gamma:  beta(t) = (1 - 1/t)^(gamma+1),  e(t) = beta e(t-1) + (1 - beta) theta(t),  theta(t) = the parameter AFTER the AdamW
// update of step t (what the classic EMA takes).  beta(1) = 0, so e(1) = theta(1) whatever the slab held.  The weight of theta(tau) in e(t) is
// w_tau = (1 - beta(tau)) (tau/t)^(gamma+1); the weights sum to 1.
// The kernel does no transcendental arithmetic: the caller passes c = 1 - beta(t), computed in f64 as -expm1((gamma+1) log1p(-1/t)), and the
// update is the ONE-coefficient form  e <- e + c (theta - e)  in f32.  (beta e + (1-beta) theta with two separately rounded coefficients has
// its fixed point for a constant parameter at theta (1-beta)_f32 / (1 - beta_f32): at t ~ 1e6, gamma ~ 17 that is off by ~3e-8 / 1.8e-5 =
// 0.17 %.  The one-coefficient form has the exact fixed point.)  c == 1 (t = 1) stores theta and does not read the slab: a NaN in an
// uninitialised slab would survive 1 * (theta - NaN).
// p, m, v, ema: the operations of adamw_ema_kernel, in its order -- turning tracks on never perturbs training (tested bitwise).
struct TrackArgs { float* e[4]; float c[4]; };
// One element of adamw_ema_kernel.  Its expressions are compiled with floating-point contraction on, and which product of `x * a + b * y`
// joins the addition is the compiler's choice: there it is always the first (read off the kernel's code: m = fma(w1, g - m, m), v = fma(v,
// beta2, w2 * (g * g)), p = fma(p, decay_mul, neg_step * (m / denom)), ema = fma(ema, ema_d, ema_a * p)); in another loop shape it may be
// the other one, and the result then differs in the last bit.  So the same operations are written out here with contraction off: the
// 16-byte loop and the scalar loop below both give adamw_ema_kernel's bits (tested bitwise, also off 16-byte boundaries).
__device__ __forceinline__ void adamw_ema_elem(float& p, float g, float& m, float& v, float& e, const AdamArgs& a) {
#pragma clang fp contract(off)
  const float gj = a.gscale == 1.f ? g : g * a.gscale;
  m = __builtin_fmaf(a.w1, gj - m, m);                              // exp_avg.lerp_(grad, 1-beta1)
  const float g2 = gj * gj;
  v = __builtin_fmaf(v, a.beta2, a.w2 * g2);                        // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;                // (sqrt(v)/bc2_sqrt).add_(eps)
  p = __builtin_fmaf(p, a.decay_mul, a.neg_step * (m / denom));     // p.mul_(1 - lr*wd); p.addcdiv_(m, denom, value=-step_size)
  e = __builtin_fmaf(e, a.ema_d, a.ema_a * p);
}
// e + c (theta - e), as one subtraction and one fma in both loops: a track's bits do not depend on where its slab starts
__device__ __forceinline__ float track_elem(float e, float c, float theta) {
#pragma clang fp contract(off)
  return __builtin_fmaf(c, theta - e, e);
}
// ADAM = false: the tracks alone (p is only read).  Elements [head, head + 4 nvec) go as 16-byte vectors; the scalar loop takes the head
// (up to the first 16-byte boundary) and the tail -- or everything, when the slabs are not congruent modulo 16 bytes (head = n).
template <int K, bool ADAM>
__global__ void adamw_ema_tracks_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                        float* __restrict__ ema, long n, long head, AdamArgs a, TrackArgs t) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
  const long nvec = (n - head) / 4, tail0 = head + nvec * 4, nscalar = head + (n - tail0);
  for (long q = tid; q < nvec; q += nthreads) {
    const long i = head + q * 4;
    const float4 pv = *(const float4*)(p + i);
    float pa[4] = {pv.x, pv.y, pv.z, pv.w};
    if (ADAM) {
      float4 gv = *(const float4*)(g + i), mv = *(float4*)(m + i), vv = *(float4*)(v + i);
      float ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
      float ea[4] = {0, 0, 0, 0};
      if (ema) { float4 e = *(float4*)(ema + i); ea[0] = e.x; ea[1] = e.y; ea[2] = e.z; ea[3] = e.w; }
#pragma unroll
      for (int j = 0; j < 4; ++j) adamw_ema_elem(pa[j], ga[j], ma[j], va[j], ea[j], a);
      *(float4*)(p + i) = make_float4(pa[0], pa[1], pa[2], pa[3]);
      *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
      if (ema) *(float4*)(ema + i) = make_float4(ea[0], ea[1], ea[2], ea[3]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float4 o = make_float4(pa[0], pa[1], pa[2], pa[3]);
      if (t.c[k] != 1.f) {
        const float4 e = *(const float4*)(t.e[k] + i);
        o.x = track_elem(e.x, t.c[k], pa[0]); o.y = track_elem(e.y, t.c[k], pa[1]);
        o.z = track_elem(e.z, t.c[k], pa[2]); o.w = track_elem(e.w, t.c[k], pa[3]);
      }
      *(float4*)(t.e[k] + i) = o;
    }
  }
  for (long s = tid; s < nscalar; s += nthreads) {
    const long i = s < head ? s : tail0 + (s - head);
    float ps = p[i];
    if (ADAM) {
      float ms = m[i], vs = v[i], es = ema ? ema[i] : 0.f;
      adamw_ema_elem(ps, g[i], ms, vs, es, a);
      p[i] = ps; m[i] = ms; v[i] = vs;
      if (ema) ema[i] = es;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float o = ps;
      if (t.c[k] != 1.f) o = track_elem(t.e[k][i], t.c[k], ps);
      t.e[k][i] = o;
    }
  }
}
// head (in elements) of the scalar prologue: up to the first 16-byte boundary when every slab has the same address modulo 16, else n
static long tracks_head(const void* const* ptrs, int count, long n) {
  const unsigned long r = (unsigned long)ptrs[0] & 15ul;
  for (int i = 1; i < count; ++i)
    if (((unsigned long)ptrs[i] & 15ul) != r) return n;
  const long h = (long)((16ul - r) & 15ul) / 4;
  return h < n ? h : n;
}
template <bool ADAM>
static int launch_tracks(float* p, const float* g, float* m, float* v, float* ema, long n, const AdamArgs& a, int ntracks, float* const* ts,
                         const double* cs, void* stream, const char* name) {
  LDMAE_REQUIRE(ntracks >= 1 && ntracks <= 4, "%s: %d tracks (1..4)", name, ntracks);
  TrackArgs t;
  const void* ptrs[9];
  int np = 0;
  ptrs[np++] = p;
  if (ADAM) { ptrs[np++] = g; ptrs[np++] = m; ptrs[np++] = v; if (ema) ptrs[np++] = ema; }
  for (int k = 0; k < 4; ++k) { t.e[k] = nullptr; t.c[k] = 0.f; }
  for (int k = 0; k < ntracks; ++k) {
    LDMAE_REQUIRE(ts[k] != nullptr, "%s: track %d has no slab", name, k);
    LDMAE_REQUIRE(cs[k] > 0.0 && cs[k] <= 1.0, "%s: track %d coefficient %g is not 1 - beta(t) in (0, 1]", name, k, cs[k]);
    t.e[k] = ts[k];
    t.c[k] = (float)cs[k];
    LDMAE_REQUIRE(t.c[k] > 0.f, "%s: track %d coefficient %g rounds to 0 in f32", name, k, cs[k]);
    ptrs[np++] = ts[k];
  }
  for (int i = 0; i < np; ++i) LDMAE_REQUIRE(((unsigned long)ptrs[i] & 3ul) == 0, "%s: a slab is not 4-byte aligned", name);
  const long head = tracks_head(ptrs, np, n), nvec = (n - head) / 4, nscalar = n - nvec * 4;
  const dim3 grid(ew_grid(nvec > nscalar ? nvec : nscalar)), block(256);
  hipStream_t st = as_stream(stream);
  switch (ntracks) {
    case 1: hipLaunchKernelGGL((adamw_ema_tracks_kernel<1, ADAM>), grid, block, 0, st, p, g, m, v, ema, n, head, a, t); break;
    case 2: hipLaunchKernelGGL((adamw_ema_tracks_kernel<2, ADAM>), grid, block, 0, st, p, g, m, v, ema, n, head, a, t); break;
    case 3: hipLaunchKernelGGL((adamw_ema_tracks_kernel<3, ADAM>), grid, block, 0, st, p, g, m, v, ema, n, head, a, t); break;
    default: hipLaunchKernelGGL((adamw_ema_tracks_kernel<4, ADAM>), grid, block, 0, st, p, g, m, v, ema, n, head, a, t); break;
  }
  LDMAE_CHECK_LAUNCH(name);
  return LDMAE_OK;
}
extern "C" int ldmae_adamw_ema_tracks(float* p, const float* g, float* m, float* v, float* ema, long n, int step, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, double ema_decay, double grad_scale, int ntracks,
                                      float* t0, float* t1, float* t2, float* t3, double c0, double c1, double c2, double c3, void* stream) {
  LDMAE_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw_ema_tracks: bad arguments");
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  AdamArgs a;                                    // as ldmae_adamw_ema prepares them
  a.decay_mul = (float)(1.0 - lr * weight_decay);
  a.w1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.w2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)eps;
  a.neg_step = (float)(-(lr / bc1));
  a.ema_d = (float)ema_decay;
  a.ema_a = (float)(1.0 - ema_decay);
  a.gscale = (float)grad_scale;
  float* const ts[4] = {t0, t1, t2, t3};
  const double cs[4] = {c0, c1, c2, c3};
  return launch_tracks<true>(p, g, m, v, ema, n, a, ntracks, ts, cs, stream, "adamw_ema_tracks");
}
extern "C" int ldmae_ema_tracks_only(const float* p, long n, int ntracks, float* t0, float* t1, float* t2, float* t3, double c0, double c1,
                                     double c2, double c3, void* stream) {
  LDMAE_REQUIRE(p && n > 0, "ema_tracks_only: bad arguments");
  float* const ts[4] = {t0, t1, t2, t3};
  const double cs[4] = {c0, c1, c2, c3};
  AdamArgs a = {};
  return launch_tracks<false>(const_cast<float*>(p), nullptr, nullptr, nullptr, nullptr, n, a, ntracks, ts, cs, stream, "ema_tracks_only");
}

// ------------------------------------------------------------------ combination of snapshots: sum_i x_i snapshot_i
// The least-squares coefficients have mixed signs and run to ~3.7 in magnitude for narrow targets, so the sum is kept in f64 and rounded
// to f32 once, at the end.  16-byte accesses where both buffers allow them, a scalar tail (or everything) otherwise.
__global__ void snapshot_accumulate_kernel(double* __restrict__ acc, const float* __restrict__ x, long n, long nvec, double coef) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
  for (long q = tid; q < nvec; q += nthreads) {
    const float4 xv = *(const float4*)(x + q * 4);
    double2 a0 = *(double2*)(acc + q * 4), a1 = *(double2*)(acc + q * 4 + 2);
    a0.x += coef * (double)xv.x; a0.y += coef * (double)xv.y; a1.x += coef * (double)xv.z; a1.y += coef * (double)xv.w;
    *(double2*)(acc + q * 4) = a0; *(double2*)(acc + q * 4 + 2) = a1;
  }
  for (long i = nvec * 4 + tid; i < n; i += nthreads) acc[i] += coef * (double)x[i];
}
__global__ void snapshot_finish_kernel(float* __restrict__ out, const double* __restrict__ acc, long n, long nvec) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
  for (long q = tid; q < nvec; q += nthreads) {
    const double2 a0 = *(const double2*)(acc + q * 4), a1 = *(const double2*)(acc + q * 4 + 2);
    *(float4*)(out + q * 4) = make_float4((float)a0.x, (float)a0.y, (float)a1.x, (float)a1.y);
  }
  for (long i = nvec * 4 + tid; i < n; i += nthreads) out[i] = (float)acc[i];
}
extern "C" int ldmae_snapshot_accumulate(double* acc, const float* x, long n, double coef, void* stream) {
  LDMAE_REQUIRE(acc && x && n > 0, "snapshot_accumulate: bad arguments");
  LDMAE_REQUIRE(((unsigned long)acc & 7ul) == 0 && ((unsigned long)x & 3ul) == 0, "snapshot_accumulate: misaligned buffer");
  LDMAE_REQUIRE(coef == coef && coef - coef == 0.0, "snapshot_accumulate: coefficient %g is not finite", coef);
  const long nvec = (((unsigned long)acc | (unsigned long)x) & 15ul) == 0 ? n / 4 : 0;
  hipLaunchKernelGGL(snapshot_accumulate_kernel, dim3(ew_grid(nvec ? nvec : n)), dim3(256), 0, as_stream(stream), acc, x, n, nvec, coef);
  LDMAE_CHECK_LAUNCH("snapshot_accumulate");
  return LDMAE_OK;
}
extern "C" int ldmae_snapshot_finish(float* out, const double* acc, long n, void* stream) {
  LDMAE_REQUIRE(out && acc && n > 0, "snapshot_finish: bad arguments");
  LDMAE_REQUIRE(((unsigned long)acc & 7ul) == 0 && ((unsigned long)out & 3ul) == 0, "snapshot_finish: misaligned buffer");
  const long nvec = (((unsigned long)acc | (unsigned long)out) & 15ul) == 0 ? n / 4 : 0;
  hipLaunchKernelGGL(snapshot_finish_kernel, dim3(ew_grid(nvec ? nvec : n)), dim3(256), 0, as_stream(stream), out, acc, n, nvec);
  LDMAE_CHECK_LAUNCH("snapshot_finish");
  return LDMAE_OK;
}
