// Linear-probe and k-NN evaluation of tokenizer features (ldmae_amd/linear_probe.py): the token pool, MAE's probe head
// (BatchNorm1d without affine -> Linear; the Linear runs on the f32 GEMMs of gemm.hip), softmax cross-entropy with the rank of the true class,
// the LARS update of the reference's util/lars.py, and the two kernels of the k-NN classifier (top-k merge of similarity chunks, weighted vote).
// No atomics anywhere: every sum has one fixed order, so two launches on the same inputs give the same bits.
#include "common.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------- token_mean: out[b, d] = (1 / N) sum_n x[b, n, col0 + d]
// A block owns 16 columns of one sample; 16 row groups of 16 lanes each add rows g, g + 16, ... in ascending order, thread g = 0 adds the 16
// group sums in ascending order and divides once.
constexpr int TM_COLS = 16, TM_GROUPS = 16;
template <typename T>
__global__ __launch_bounds__(256) void token_mean_kernel(const T* __restrict__ x, long ldx, int col0, float* __restrict__ out, int N, int D, int tiles) {
  __shared__ float part[TM_GROUPS][TM_COLS + 1];
  const int b = blockIdx.x / tiles, c = threadIdx.x & (TM_COLS - 1), g = threadIdx.x / TM_COLS, d = (blockIdx.x % tiles) * TM_COLS + c;
  float s = 0.f;
  if (d < D) {
    const T* p = x + (long)b * N * ldx + col0 + d;
    for (int n = g; n < N; n += TM_GROUPS) s += to_f<T>(p[(long)n * ldx]);
  }
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && d < D) {
    float t = part[0][c];
    for (int i = 1; i < TM_GROUPS; ++i) t += part[i][c];
    out[(long)b * D + d] = t / (float)N;
  }
}

// ---------------------------------------------------------------- bn1d_fwd: BatchNorm1d(affine = False) over the batch
// A block owns 32 columns (one 128-B line per row); 8 row groups.  Two passes: the column sum, then sum (x - mean)^2 with the f32 mean the
// kernel normalises with -- never E[x^2] - mean^2.  Both sums are accumulated in f64 (f32 data, exact squares), so the statistics carry the
// roundings of their f32 results only.
constexpr int BN_COLS = 32, BN_GROUPS = 8;
__global__ __launch_bounds__(256) void bn1d_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ xhat, int ldo, float* run_mean,
                                                       float* run_var, float* save_mean, float* save_rstd, int B, int D, float eps, float momentum,
                                                       int training) {
  __shared__ double part[BN_GROUPS][BN_COLS + 1];
  __shared__ float stat[2][BN_COLS];
  const int c = threadIdx.x & (BN_COLS - 1), g = threadIdx.x / BN_COLS, d = blockIdx.x * BN_COLS + c;
  const bool ok = d < D;
  float mean = 0.f, rstd = 0.f;
  if (training) {
    double s = 0.0;
    if (ok)
      for (int n = g; n < B; n += BN_GROUPS) s += (double)x[(long)n * ldx + d];
    part[g][c] = s;
    __syncthreads();
    if (g == 0) {
      double t = part[0][c];
      for (int i = 1; i < BN_GROUPS; ++i) t += part[i][c];
      stat[0][c] = (float)(t / (double)B);
    }
    __syncthreads();
    mean = stat[0][c];
    double q = 0.0;
    if (ok)
      for (int n = g; n < B; n += BN_GROUPS) {
        const float e = x[(long)n * ldx + d] - mean;
        q += (double)e * (double)e;
      }
    part[g][c] = q;
    __syncthreads();
    if (g == 0) {
      double t = part[0][c];
      for (int i = 1; i < BN_GROUPS; ++i) t += part[i][c];
      const float var = (float)(t / (double)B);
      const float r = 1.f / sqrtf(var + eps);
      stat[1][c] = r;
      if (ok) {
        const float keep = 1.f - momentum;
        run_mean[d] = fmaf(momentum, mean, keep * run_mean[d]);
        run_var[d] = fmaf(momentum, (float)(t / (double)(B - 1)), keep * run_var[d]);
        if (save_mean) save_mean[d] = mean;
        if (save_rstd) save_rstd[d] = r;
      }
    }
    __syncthreads();
    rstd = stat[1][c];
  } else if (ok) {
    mean = run_mean[d];
    rstd = 1.f / sqrtf(run_var[d] + eps);
  }
  if (ok)
    for (int n = g; n < B; n += BN_GROUPS) xhat[(long)n * ldo + d] = (x[(long)n * ldx + d] - mean) * rstd;
}

// ---------------------------------------------------------------- softmax_xent: loss, dlogits and the rank of the true class of one row per block
// R > 0: the row is read ONCE into R registers per thread (C <= 256 R); R = 0: three passes over the row in global memory (the second and
// third hit the cache).  rank counts comparisons of the given f32 logits only.  A label outside [0, C) (the host wrapper refuses them) reads
// nothing: loss = NaN, rank = -1, a zero gradient row.
template <int R>
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                           float* __restrict__ loss, float* __restrict__ dlogits, int ldd, int* __restrict__ rank,
                                                           int C, float grad_scale) {
  __shared__ float redf[4];
  __shared__ int redi[4];
  constexpr bool REG = R > 0;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* l = logits + (long)row * ld;
  float* dl = dlogits ? dlogits + (long)row * ldd : nullptr;
  const long long y = labels[row];
  if (y < 0 || y >= (long long)C) {
    if (tid == 0) { loss[row] = __builtin_nanf(""); rank[row] = -1; }
    if (dl)
      for (int c = tid; c < C; c += 256) dl[c] = 0.f;
    return;
  }
  const float ly = l[y];
  const int iters = REG ? R : (C + 255) / 256;
  float v[REG ? R : 1];
  float m = -__builtin_inff();
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int c = tid + 256 * i;
    const float xv = c < C ? l[c] : -__builtin_inff();
    if (REG) v[REG ? i : 0] = xv;
    m = fmaxf(m, xv);
    cnt += (c < C && (xv > ly || (xv == ly && c < (int)y))) ? 1 : 0;
  }
  m = block_max(m, redf);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int c = tid + 256 * i;
    const float xv = REG ? v[REG ? i : 0] : (c < C ? l[c] : -__builtin_inff());
    const float e = c < C ? expf(xv - m) : 0.f;
    if (REG) v[REG ? i : 0] = e;
    s += e;
  }
  s = block_sum(s, redf);
  cnt = block_sum(cnt, redi);
  if (tid == 0) {
    loss[row] = (m + logf(s)) - ly;
    rank[row] = cnt;
  }
  if (dl) {
#pragma unroll
    for (int i = 0; i < iters; ++i) {
      const int c = tid + 256 * i;
      if (c < C) {
        const float e = REG ? v[REG ? i : 0] : expf(l[c] - m);
        const float p = e / s;
        dl[c] = (c == (int)y ? p - 1.f : p) * grad_scale;
      }
    }
  }
}

// ---------------------------------------------------------------- LARS (util/lars.py): norms in two stages, then the step
// Stage 1: a block adds p^2 and dp^2 (dp = g + wd p, as the step kernel forms it) of 4096 elements in f64 and stores the two sums; stage 2: one
// block adds the partials in ascending order per thread, joins, and stores (|p|, |dp|) as f32.  The step kernel reads them from device memory.
constexpr int LARS_PER_BLOCK = 4096;
__global__ __launch_bounds__(256) void lars_norms1_kernel(const float* __restrict__ p, const float* __restrict__ g, long n, float wd, double* __restrict__ part) {
  __shared__ double red[4];
  const long base = (long)blockIdx.x * LARS_PER_BLOCK;
  double sp = 0.0, sd = 0.0;
#pragma unroll 4
  for (int i = 0; i < LARS_PER_BLOCK / 256; ++i) {
    const long j = base + i * 256 + threadIdx.x;
    if (j < n) {
      const float pv = p[j], dp = fmaf(wd, pv, g[j]);
      sp += (double)pv * (double)pv;
      sd += (double)dp * (double)dp;
    }
  }
  sp = block_sum(sp, red);
  sd = block_sum(sd, red);
  if (threadIdx.x == 0) { part[2 * (long)blockIdx.x] = sp; part[2 * (long)blockIdx.x + 1] = sd; }
}
__global__ __launch_bounds__(256) void lars_norms2_kernel(const double* __restrict__ part, int nblk, float* __restrict__ norms) {
  __shared__ double red[4];
  double sp = 0.0, sd = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) { sp += part[2 * (long)j]; sd += part[2 * (long)j + 1]; }
  sp = block_sum(sp, red);
  sd = block_sum(sd, red);
  if (threadIdx.x == 0) { norms[0] = (float)sqrt(sp); norms[1] = (float)sqrt(sd); }
}
// norms != NULL: a tensor of more than one dimension (weight decay and the trust ratio apply); NULL: a bias (neither does)
__global__ __launch_bounds__(256) void lars_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu, long n,
                                                        const float* __restrict__ norms, float lr, float wd, float momentum, float trust) {
  float q = 1.f;
  if (norms) {
    const float pn = norms[0], un = norms[1];
    if (pn > 0.f && un > 0.f) q = trust * pn / un;
  }
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float pv = p[j];
  float dp = g[j];
  if (norms) dp = fmaf(wd, pv, dp) * q;
  const float m = fmaf(momentum, mu[j], dp);
  mu[j] = m;
  p[j] = fmaf(-lr, m, pv);
}

// ---------------------------------------------------------------- l2_normalize: out[m, :] = x[m, :] / max(sqrtf(sq[m]), 1e-12) (F.normalize)
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, const float* __restrict__ sq, float* __restrict__ out, long n, int D) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = x[j] / fmaxf(sqrtf(sq[j / D]), 1e-12f);
}

// ---------------------------------------------------------------- topk_merge: a chunk of similarities into per-query sorted lists
// One block per query.  Order: a valid entry (index >= 0) before an empty slot; among valid ones the larger value first, equal values by
// ascending index -- comparisons only.  The list (k <= 256 slots) sits in the first half of a 512-entry LDS array, candidates that beat the
// current k-th entry are appended to the second half, and a bitonic sort of the 512 entries folds them in whenever the next 256 columns might
// not fit.  A NaN similarity is never a candidate.
__device__ __forceinline__ bool tk_before(float av, int ai, float bv, int bi) {
  if (ai < 0 || bi < 0) return ai >= 0 && bi < 0;
  return av > bv || (av == bv && ai < bi);
}
__device__ __forceinline__ void tk_sort512(float* kv, int* ki) {
  const int t = threadIdx.x;
  for (int size = 2; size <= 512; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int i = 2 * t - (t & (stride - 1)), j = i + stride;
      const float av = kv[i], bv = kv[j];
      const int ai = ki[i], bi = ki[j];
      const bool up = (i & size) == 0;                    // this run is sorted best-first; the next one worst-first
      if (up ? tk_before(bv, bi, av, ai) : tk_before(av, ai, bv, bi)) { kv[i] = bv; ki[i] = bi; kv[j] = av; ki[j] = ai; }
    }
  __syncthreads();
}
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ sims, int lds, int Nc, int col0, float* __restrict__ vals,
                                                         int* __restrict__ idx, int k) {
  __shared__ float kv[512];
  __shared__ int ki[512];
  __shared__ int wcnt[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long q = blockIdx.x;
  const float* srow = sims + q * lds;
  kv[t] = t < k ? vals[q * k + t] : -__builtin_inff();
  ki[t] = t < k ? idx[q * k + t] : -1;
  kv[256 + t] = -__builtin_inff();
  ki[256 + t] = -1;
  __syncthreads();
  float thv = kv[k - 1];
  int thi = ki[k - 1];
  int cnt = 0;                                            // candidates waiting in the second half (the same in every thread)
  for (int c0 = 0; c0 < Nc; c0 += 256) {
    const int c = c0 + t;
    const float v = c < Nc ? srow[c] : 0.f;
    bool cand = c < Nc && v == v && tk_before(v, col0 + c, thv, thi);
    unsigned long long mask = __ballot(cand);
    if (lane == 0) wcnt[w] = __popcll(mask);
    __syncthreads();
    int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (cnt + total > 256) {                              // (the same in every thread) they do not fit beside the waiting ones: fold those in first
      tk_sort512(kv, ki);                                 // ends with a barrier: wcnt has been read by everyone
      thv = kv[k - 1]; thi = ki[k - 1];
      __syncthreads();
      kv[256 + t] = -__builtin_inff(); ki[256 + t] = -1;
      cnt = 0;
      cand = cand && tk_before(v, col0 + c, thv, thi);    // against the new k-th entry
      mask = __ballot(cand);
      if (lane == 0) wcnt[w] = __popcll(mask);
      __syncthreads();
      total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    int off = cnt;
    for (int i = 0; i < w; ++i) off += wcnt[i];
    if (cand) {
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
      kv[256 + pos] = v;
      ki[256 + pos] = col0 + c;
    }
    cnt += total;
    __syncthreads();                                      // wcnt is rewritten by the next round
  }
  if (cnt > 0) tk_sort512(kv, ki);
  if (t < k) { vals[q * k + t] = kv[t]; idx[q * k + t] = ki[t]; }
}

// ---------------------------------------------------------------- knn_vote: class scores in LDS, the rank of the true class
// One block per query: threads j < k form w_j = exp(sim_j / T) and look the neighbour's label up; thread 0 adds them into the scores in list
// order; every thread then counts the classes that beat the true one (the rank rule of softmax_xent).  Dynamic LDS: C scores.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ vals, const int* __restrict__ idx, int k,
                                                       const long long* __restrict__ bank_labels, int nbank, const long long* __restrict__ qlabels,
                                                       int C, float inv_t, int* __restrict__ rank, float* __restrict__ scores_out) {
  extern __shared__ float scores[];
  __shared__ float wv[256];
  __shared__ int wl[256];
  __shared__ int redi[4];
  const int t = threadIdx.x;
  const long q = blockIdx.x;
  for (int c = t; c < C; c += 256) scores[c] = 0.f;
  int lab = -1;
  float wgt = 0.f;
  if (t < k) {
    const int j = idx[q * k + t];
    if (j >= 0 && j < nbank) {
      const long long bl = bank_labels[j];
      if (bl >= 0 && bl < (long long)C) { lab = (int)bl; wgt = expf(vals[q * k + t] * inv_t); }
    }
  }
  wv[t] = wgt;
  wl[t] = lab;
  __syncthreads();
  if (t == 0)
    for (int j = 0; j < k; ++j)
      if (wl[j] >= 0) scores[wl[j]] += wv[j];
  __syncthreads();
  const long long y = qlabels[q];
  if (scores_out)
    for (int c = t; c < C; c += 256) scores_out[q * C + c] = scores[c];
  if (y < 0 || y >= (long long)C) {
    if (t == 0) rank[q] = -1;
    return;
  }
  const float sy = scores[y];
  int cnt = 0;
  for (int c = t; c < C; c += 256) {
    const float sc = scores[c];
    cnt += (sc > sy || (sc == sy && c < (int)y)) ? 1 : 0;
  }
  cnt = block_sum(cnt, redi);
  if (t == 0) rank[q] = cnt;
}

}  // namespace

extern "C" int ldmae_token_mean(int dtype, const void* x, long ldx, int col0, float* out, int B, int N, int D, void* stream) {
  LDMAE_REQUIRE(x && out, "token_mean: null pointer");
  LDMAE_REQUIRE(B > 0 && N > 0 && D > 0 && col0 >= 0 && ldx >= (long)col0 + D, "token_mean: B=%d N=%d D=%d col0=%d ldx=%ld (need col0 + D <= ldx)", B, N, D,
                col0, ldx);
  const int tiles = (int)cdiv(D, TM_COLS);
  LDMAE_REQUIRE((long)B * tiles < (1l << 31), "token_mean: B=%d x %d column tiles exceed the grid", B, tiles);
  const bool known = dtype_dispatch<float, bf16, f16>(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    hipLaunchKernelGGL(token_mean_kernel<T>, dim3((unsigned)(B * tiles)), dim3(256), 0, as_stream(stream), (const T*)x, ldx, col0, out, N, D, tiles);
  });
  LDMAE_REQUIRE(known, "token_mean: dtype %d (f32, bf16 or fp16)", dtype);
  LDMAE_CHECK_LAUNCH("token_mean");
  return LDMAE_OK;
}

extern "C" int ldmae_bn1d_fwd(int dtype, const void* x, int ldx, void* xhat, int ldo, float* run_mean, float* run_var, float* save_mean,
                              float* save_rstd, int B, int D, float eps, float momentum, int training, void* stream) {
  LDMAE_REQUIRE(x && xhat && run_mean && run_var, "bn1d_fwd: null pointer");
  LDMAE_REQUIRE(B > 0 && D > 0 && ldx >= D && ldo >= D, "bn1d_fwd: B=%d D=%d ldx=%d ldo=%d", B, D, ldx, ldo);
  LDMAE_REQUIRE(!training || B > 1, "bn1d_fwd: training statistics need more than one row (B=%d)", B);
  LDMAE_REQUIRE(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "bn1d_fwd: eps=%g momentum=%g", (double)eps, (double)momentum);
  const bool known = dtype_dispatch<float>(dtype, [&](auto) {
    hipLaunchKernelGGL(bn1d_fwd_kernel, dim3(cdiv(D, BN_COLS)), dim3(256), 0, as_stream(stream), (const float*)x, ldx, (float*)xhat, ldo, run_mean,
                       run_var, save_mean, save_rstd, B, D, eps, momentum, training);
  });
  LDMAE_REQUIRE(known, "bn1d_fwd: dtype %d (f32 only)", dtype);
  LDMAE_CHECK_LAUNCH("bn1d_fwd");
  return LDMAE_OK;
}

extern "C" int ldmae_softmax_xent(int dtype, const void* logits, int ld, const long long* labels, float* loss, void* dlogits, int ldd, int* rank,
                                  int B, int C, float grad_scale, void* stream) {
  LDMAE_REQUIRE(logits && labels && loss && rank, "softmax_xent: null pointer");
  LDMAE_REQUIRE(B > 0 && C > 0 && ld >= C && (!dlogits || ldd >= C), "softmax_xent: B=%d C=%d ld=%d ldd=%d", B, C, ld, ldd);
  const bool known = dtype_dispatch<float>(dtype, [&](auto) {
    auto go = [&](auto r) {
      hipLaunchKernelGGL(softmax_xent_kernel<decltype(r)::value>, dim3((unsigned)B), dim3(256), 0, as_stream(stream), (const float*)logits, ld, labels,
                         loss, (float*)dlogits, ldd, rank, C, grad_scale);
    };
    if (C <= 256) go(IC<1>{}); else if (C <= 1024) go(IC<4>{}); else if (C <= 4096) go(IC<16>{}); else go(IC<0>{});
  });
  LDMAE_REQUIRE(known, "softmax_xent: dtype %d (f32 only)", dtype);
  LDMAE_CHECK_LAUNCH("softmax_xent");
  return LDMAE_OK;
}

extern "C" long ldmae_lars_workspace_bytes(long n) { return n > 0 ? 16l * (long)cdiv(n, LARS_PER_BLOCK) : 0; }

extern "C" int ldmae_lars_norms(int dtype, const void* p, const void* g, long n, float wd, void* workspace, float* norms, void* stream) {
  LDMAE_REQUIRE(p && g && workspace && norms, "lars_norms: null pointer");
  LDMAE_REQUIRE(n > 0 && n <= (long)LARS_PER_BLOCK * 0x7fffffffl, "lars_norms: n=%ld", n);
  LDMAE_REQUIRE(((uintptr_t)workspace & 7) == 0, "lars_norms: the workspace must be 8-byte aligned");
  const unsigned nblk = cdiv(n, LARS_PER_BLOCK);
  const bool known = dtype_dispatch<float>(dtype, [&](auto) {
    hipLaunchKernelGGL(lars_norms1_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), (const float*)p, (const float*)g, n, wd, (double*)workspace);
    hipLaunchKernelGGL(lars_norms2_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const double*)workspace, (int)nblk, norms);
  });
  LDMAE_REQUIRE(known, "lars_norms: dtype %d (f32 only)", dtype);
  LDMAE_CHECK_LAUNCH("lars_norms");
  return LDMAE_OK;
}

extern "C" int ldmae_lars_step(int dtype, void* p, const void* g, void* mu, long n, const float* norms, float lr, float wd, float momentum,
                               float trust, void* stream) {
  LDMAE_REQUIRE(p && g && mu, "lars_step: null pointer");
  LDMAE_REQUIRE(n > 0 && n <= 256l * 0x7fffffffl, "lars_step: n=%ld", n);
  const bool known = dtype_dispatch<float>(dtype, [&](auto) {
    hipLaunchKernelGGL(lars_step_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), (float*)p, (const float*)g, (float*)mu, n, norms, lr, wd,
                       momentum, trust);
  });
  LDMAE_REQUIRE(known, "lars_step: dtype %d (f32 only)", dtype);
  LDMAE_CHECK_LAUNCH("lars_step");
  return LDMAE_OK;
}

extern "C" int ldmae_l2_normalize(const float* x, const float* sqnorms, float* out, long M, int D, void* stream) {
  LDMAE_REQUIRE(x && sqnorms && out, "l2_normalize: null pointer");
  LDMAE_REQUIRE(M > 0 && D > 0 && M * D <= 256l * 0x7fffffffl, "l2_normalize: M=%ld D=%d", M, D);
  hipLaunchKernelGGL(l2_normalize_kernel, dim3(cdiv(M * D, 256)), dim3(256), 0, as_stream(stream), x, sqnorms, out, M * D, D);
  LDMAE_CHECK_LAUNCH("l2_normalize");
  return LDMAE_OK;
}

extern "C" int ldmae_topk_merge(const float* sims, int ld, int M, int Nc, int col0, float* vals, int* idx, int k, void* stream) {
  LDMAE_REQUIRE(sims && vals && idx, "topk_merge: null pointer");
  LDMAE_REQUIRE(k >= 1 && k <= LDMAE_TOPK_MAX_K, "topk_merge: k=%d (1 .. LDMAE_TOPK_MAX_K = %d)", k, LDMAE_TOPK_MAX_K);
  LDMAE_REQUIRE(M > 0 && Nc > 0 && ld >= Nc && col0 >= 0 && (long)col0 + Nc <= 0x7fffffffl, "topk_merge: M=%d Nc=%d ld=%d col0=%d", M, Nc, ld, col0);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(256), 0, as_stream(stream), sims, ld, Nc, col0, vals, idx, k);
  LDMAE_CHECK_LAUNCH("topk_merge");
  return LDMAE_OK;
}

extern "C" int ldmae_knn_vote(const float* vals, const int* idx, int M, int k, const long long* bank_labels, int nbank, const long long* qlabels,
                              int C, float temperature, int* rank, float* scores, void* stream) {
  LDMAE_REQUIRE(vals && idx && bank_labels && qlabels && rank, "knn_vote: null pointer");
  LDMAE_REQUIRE(k >= 1 && k <= LDMAE_TOPK_MAX_K, "knn_vote: k=%d (1 .. LDMAE_TOPK_MAX_K = %d)", k, LDMAE_TOPK_MAX_K);
  LDMAE_REQUIRE(C >= 1 && C <= LDMAE_KNN_VOTE_MAX_C, "knn_vote: C=%d classes; the scores of a query are held in LDS, LDMAE_KNN_VOTE_MAX_C = %d fit", C,
                LDMAE_KNN_VOTE_MAX_C);
  LDMAE_REQUIRE(M > 0 && nbank > 0 && temperature > 0.f, "knn_vote: M=%d nbank=%d T=%g", M, nbank, (double)temperature);
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)M), dim3(256), (size_t)C * 4, as_stream(stream), vals, idx, k, bank_labels, nbank, qlabels, C,
                     1.f / temperature, rank, scores);
  LDMAE_CHECK_LAUNCH("knn_vote");
  return LDMAE_OK;
}
