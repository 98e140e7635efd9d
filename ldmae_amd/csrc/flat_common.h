// The two access patterns of the "flat" f32 kernels (ode.hip: the dopri5 / likelihood / SDE sampler arithmetic; fm_valid.hip: the validation
// loss), each written once: a walk over n floats as float4 items plus a scalar tail, and a two-stage fixed-order reduction of [B, m] rows.
//
// NO ARITHMETIC ON VALUES lives here.  ode.hip compiles with hipcc's default contraction (and spells the fused operations it relies on),
// fm_valid.hip under `#pragma clang fp contract(off)`; a pragma does not reach a header included before it, so a multiply written here, or
// an add here that consumed a functor's product, could be fused in one file's kernels and not in the other's.  This header loads, stores,
// counts, and adds partial sums (s += partial[i], block_sum of common.h); every product and every term of a sum is the including file's
// functor, which takes the running sum and returns the new one.
#pragma once
#include "common.h"

constexpr int FLAT_THREADS = 256;
constexpr int FLAT_UNROLL = 4;                                   // items per thread
constexpr long FLAT_BLOCK_ITEMS = (long)FLAT_THREADS * FLAT_UNROLL;

// ---------------------------------------------------------------- the walker
// Item v < n / 4 is the float4 at element 4 v; item n / 4 (present when n % 4 != 0) is the scalar tail of n % 4 elements.  A block of 256
// threads owns 1024 consecutive items, thread t the items t, t + 256, t + 512, t + 768 of them, so the grid is cdiv(items, 1024): a function
// of n alone, never of the device.
inline long ode_items(long n) { return (n >> 2) + ((n & 3) ? 1 : 0); }
inline unsigned ode_grid(long n) { return cdiv(ode_items(n), FLAT_BLOCK_ITEMS); }
inline bool flat_fits_grid(long n) { return ode_items(n) <= 0x7fffffffL * FLAT_BLOCK_ITEMS; }      // the "n too large" of the entry points

// f(v, cnt, whole) for every item v of this thread, in ascending order: whole = the item is a float4 the kernel may access with 16-byte
// instructions (cnt = 4); otherwise its first cnt elements are accessed one by one: the tail, and every item when !vec (a buffer that is not
// 16-byte aligned).  The tail is the last item there is, so the one thread that owns it takes it after its whole items, outside the unrolled
// loop: the loop body is the float4 path alone (vec is a literal true, or uniform over the launch).
template <typename F> __device__ __forceinline__ void flat_walk(long n, bool vec, F&& f) {
  const long nvec = n >> 2;
  const int tail = (int)(n & 3);
  const long base = (long)blockIdx.x * FLAT_BLOCK_ITEMS + threadIdx.x;
#pragma unroll
  for (int u = 0; u < FLAT_UNROLL; ++u) {
    const long v = base + (long)u * FLAT_THREADS;
    if (v < nvec) f(v, 4, vec);
  }
  const long d = nvec - base;                                    // the tail is this thread's when d is 0, 256, 512 or 768
  if (tail && d >= 0 && d < FLAT_BLOCK_ITEMS && (d & (FLAT_THREADS - 1)) == 0) f(nvec, tail, false);
}

// item v of p into x (elements beyond cnt read as 0) and back
__device__ __forceinline__ void flat_load(const float* p, long v, int cnt, bool whole, float (&x)[4]) {
  if (whole) {
    const float4 a = ((const float4*)p)[v];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < cnt ? p[(v << 2) + j] : 0.f;
  }
}
__device__ __forceinline__ void flat_store(float* p, long v, int cnt, bool whole, const float (&x)[4]) {
  if (whole) {
    ((float4*)p)[v] = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[(v << 2) + j] = x[j];
  }
}

// the side output of a step kernel: block 0 sets the nt entries of t_out (the time vector of the next model evaluation) to `value`
__device__ __forceinline__ void flat_fill_side(float* t_out, int nt, float value) {
  if (t_out && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nt; i += FLAT_THREADS) t_out[i] = value;
}

// ---------------------------------------------------------------- out[r] = finish(sum_j term(a[r, j], b[r, j])), rows of m elements
// Stage 1: block (r, c) owns the ROW_CHUNK elements [4096 c, 4096 c + 4096) of row r.  vec (every row start of a and b aligned for a
// 4-element load): thread t takes the 4-element groups t, t + 256, t + 512, t + 768 of the chunk, element order inside each; otherwise thread
// t takes the elements t, t + 256, ... (16 of them).  s = term(a, b, s) element after element, then block_sum; partial[r * chunks + c].
// Stage 2: one block per row lets thread t add partial[t], partial[t + 256], ... of the row in that order, block_sum again, out[r] =
// finish(sum).  The order depends on (m, vec) only: two runs give the same bits.
constexpr long ROW_CHUNK = 4096;
inline long row_chunks(long m) { return cdiv(m, ROW_CHUNK); }
inline long row_partials(int B, long m) { return (B > 0 && m > 0) ? (long)B * row_chunks(m) : 0; }
inline bool row_fits_grid(int B, long m) { return (long)B * row_chunks(m) <= 0x7fffffffL; }
// a_aligned / b_aligned: the base address is aligned for a 4-element load of its type
inline int row_vec(bool a_aligned, bool b_aligned, int B, long m) { return (a_aligned && b_aligned && (B == 1 || (m & 3) == 0)) ? 1 : 0; }

template <typename T, typename Term>
__global__ __launch_bounds__(FLAT_THREADS) void row_reduce_kernel(const T* __restrict__ a, const float* __restrict__ b, float* __restrict__ partial,
                                                                   long m, long chunks, int vec) {
  __shared__ float red[4];
  const Term term;
  const long r = blockIdx.x / chunks, c = blockIdx.x - r * chunks;
  const T* ar = a + r * m;
  const float* br = b + r * m;
  const long lo = c * ROW_CHUNK, hi = lo + ROW_CHUNK < m ? lo + ROW_CHUNK : m;
  float s = 0.f;
  if (vec) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long e = lo + 4 * ((long)threadIdx.x + (long)u * FLAT_THREADS);
      if (e + 4 <= hi) {
        const float4 x = load4f(ar + e), y = load4f(br + e);
        s = term(x.x, y.x, s); s = term(x.y, y.y, s); s = term(x.z, y.z, s); s = term(x.w, y.w, s);
      } else {
        for (long i = e; i < hi; ++i) s = term(to_f<T>(ar[i]), br[i], s);
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const long i = lo + threadIdx.x + (long)u * FLAT_THREADS;
      if (i < hi) s = term(to_f<T>(ar[i]), br[i], s);
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <typename Finish>
__global__ __launch_bounds__(FLAT_THREADS) void row_fold_kernel(const float* __restrict__ partial, long chunks, Finish finish, float* __restrict__ out) {
  __shared__ float red[4];
  const float* p = partial + (long)blockIdx.x * chunks;
  float s = 0.f;
  for (long i = threadIdx.x; i < chunks; i += FLAT_THREADS) s += p[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = finish(s);
}

// both stages; the caller has checked its arguments (row_fits_grid among them) and checks the launch
template <typename Term, typename T, typename Finish>
inline void row_reduce(const T* a, const float* b, float* out, int B, long m, float* partial, int vec, Finish finish, hipStream_t st) {
  const long chunks = row_chunks(m);
  hipLaunchKernelGGL((row_reduce_kernel<T, Term>), dim3((unsigned)(B * chunks)), dim3(FLAT_THREADS), 0, st, a, b, partial, m, chunks, vec);
  hipLaunchKernelGGL(row_fold_kernel<Finish>, dim3(B), dim3(FLAT_THREADS), 0, st, (const float*)partial, chunks, finish, out);
}
