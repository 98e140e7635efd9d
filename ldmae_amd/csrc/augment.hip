// Training transform of the VMAE image input on the device: RandomResizedCrop's resample (PIL crop(box).resize((S, S), BICUBIC)), the horizontal
// flip, ToTensor and Normalize, for a whole batch of packed uint8 images in ONE launch (datasets/packed_images.py draws the boxes on the host).
//
// The resample is PIL's separable one: horizontal pass, then vertical, Keys cubic (a = -0.5) stretched by fs = max(n / S, 1) per axis, taps clipped
// at the CROP BOX, weights normalised by their sum.  Everything that decides a tap set or a weight argument is done in integers, which is exact:
//   center - support + 0.5 = ((2i + 1) n + S - 4 m) / 2S,   center + support + 0.5 = ((2i + 1) n + S + 4 m) / 2S,   m = max(n, S) = S fs
//   (x - center + 0.5) / fs = ((2x + 1) S - (2i + 1) n) / 2m
// so the weight argument is ONE f32 division of two exactly represented integers (n, S <= 16384), not a chain of roundings of values near n.
//
// One workgroup makes RB output rows x TW output columns of one sample, one lane per column.  The source rows the band needs are visited in
// ascending chunks of CHT rows: the four waves run the horizontal pass of a chunk into LDS (f32, clamped to [0, 255]), then every lane adds the
// chunk's share of its vertical taps to its accumulators -- ascending chunks and ascending rows inside a chunk keep each output one ascending
// fma chain, whatever the tap count (it grows with n / S without limit).  The finished tile goes through LDS once more, mirrored if the sample
// is flipped, so that the global stores are 16-byte ones along the row.  No atomics; grid = B * ceil(S / TW) * ceil(S / RB).
#include "common.h"

namespace {
constexpr int TW = 64;            // output columns per workgroup: one per lane
constexpr int RB = 16;            // output rows per workgroup
constexpr int NW = 4;             // waves per workgroup
constexpr int CR = 8;             // source rows per wave and chunk
constexpr int CHT = NW * CR;      // source rows per chunk
constexpr int MAXN = 16384;       // largest crop side / S: keeps (2i + 1) n + S + 4 m inside 31 bits

// PIL's bicubic_filter (Resample.c), a = -0.5
__device__ __forceinline__ float keys_cubic(float t) {
  t = fabsf(t);
  if (t < 1.f) return ((1.5f * t - 2.5f) * t) * t + 1.f;
  if (t < 2.f) return (((t - 5.f) * t + 8.f) * t - 4.f) * -0.5f;
  return 0.f;
}
// taps of output index i: [lo, hi) inside [0, n)
__device__ __forceinline__ void tap_range(int i, int n, int S, int& lo, int& hi) {
  const int m = n > S ? n : S, c = (2 * i + 1) * n + S, a = c - 4 * m;
  lo = a > 0 ? a / (2 * S) : 0;
  const int b = (c + 4 * m) / (2 * S);
  hi = b < n ? b : n;
}
// un-normalised weight of tap x for output index i
__device__ __forceinline__ float tap_weight(int x, int i, int n, int S) {
  const int m = n > S ? n : S;
  return keys_cubic((float)((2 * x + 1) * S - (2 * i + 1) * n) / (float)(2 * m));
}
__device__ __forceinline__ float tap_sum(int i, int lo, int hi, int n, int S) {
  float s = 0.f;
  for (int x = lo; x < hi; ++x) s += tap_weight(x, i, n, S);
  return s;
}
__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// PER: elements per global store (1 = any S; 4 f32 / 8 bf16 = 16-byte stores, S % PER == 0 and `out` 16-byte aligned)
template <typename T, int PER>
__global__ __launch_bounds__(256) void crop_resize_flip_kernel(const unsigned char* __restrict__ blob, long blob_bytes, const long* __restrict__ offset,
                                                               const int* __restrict__ geom, T* __restrict__ out, int S, float mean, float stdv) {
  __shared__ __attribute__((aligned(16))) float hbuf[CHT * 3 * TW];      // horizontal results of one chunk [row][channel][column]; then the output tile
  __shared__ float wv[RB * CHT];                                         // normalised vertical weights of the chunk [output row][source row]
  __shared__ float vsum[RB];
  __shared__ int vlo[RB], vhi[RB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntx = (S + TW - 1) / TW, nby = (S + RB - 1) / RB;
  const int b = blockIdx.x / (ntx * nby), t = blockIdx.x % (ntx * nby);
  const int x0 = (t % ntx) * TW, y0 = (t / ntx) * RB;
  const int* g = geom + (size_t)b * 8;
  const int h = g[0], w = g[1], top = g[2], left = g[3], ch = g[4], cw = g[5], flip = g[6];
  const long off = offset[b];
  // the tables are the host's to get right (ops.crop_resize_flip checks them); a row that would read outside the blob is skipped, not followed
  // (h, w <= 2^24 keeps 3 h w far inside 63 bits: the test cannot be fooled by a wrapped product)
  if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24) || top < 0 || left < 0 || ch < 1 || cw < 1 || ch > MAXN || cw > MAXN || top > h - ch ||
      left > w - cw || off < 0 || off > blob_bytes - 3L * h * w)
    return;
  const long rs = 3L * w;
  const unsigned char* src = blob + off + ((long)top * w + left) * 3;
  const int nrv = S - y0 < RB ? S - y0 : RB, nx = S - x0 < TW ? S - x0 : TW;
  const int x = x0 + lane;
  const bool xv = lane < nx;
  int hlo = 0, hhi = 0;
  float hsum = 1.f;
  if (xv) {
    tap_range(x, cw, S, hlo, hhi);
    hsum = tap_sum(x, hlo, hhi, cw, S);
  }
  if (tid < RB) {
    int lo = 0, hi = 0;
    float s = 1.f;
    if (tid < nrv) {
      tap_range(y0 + tid, ch, S, lo, hi);
      s = tap_sum(y0 + tid, lo, hi, ch, S);
    }
    vlo[tid] = lo; vhi[tid] = hi; vsum[tid] = s;
  }
  __syncthreads();
  const int r0 = vlo[0], r1 = vhi[nrv - 1];          // tap ranges move up with the output row: the band needs source rows [r0, r1)
  float acc[RB / NW][3];
#pragma unroll
  for (int j = 0; j < RB / NW; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.f;

  for (int c0 = r0; c0 < r1; c0 += CHT) {
    const int nr = r1 - c0 < CHT ? r1 - c0 : CHT;
    for (int e = tid; e < RB * CHT; e += 256) {
      const int r = e / CHT, y = c0 + e % CHT;
      wv[e] = (y >= vlo[r] && y < vhi[r]) ? tap_weight(y, y0 + r, ch, S) / vsum[r] : 0.f;
    }
    // horizontal pass: wave `wave` takes the chunk's rows wave, wave + NW, ... (a short chunk still spreads over the four waves)
    float a[CR][3];
#pragma unroll
    for (int q = 0; q < CR; ++q) a[q][0] = a[q][1] = a[q][2] = 0.f;
    for (int k = hlo; k < hhi; ++k) {
      const float wk = tap_weight(k, x, cw, S) / hsum;
      const unsigned char* p = src + (long)c0 * rs + k * 3;
#pragma unroll
      for (int q = 0; q < CR; ++q) {
        const int row = wave + NW * q;
        if (row < nr) {
          const unsigned char* pp = p + (long)row * rs;
          a[q][0] = fmaf(wk, (float)pp[0], a[q][0]);
          a[q][1] = fmaf(wk, (float)pp[1], a[q][1]);
          a[q][2] = fmaf(wk, (float)pp[2], a[q][2]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < CR; ++q) {
      const int row = wave + NW * q;
      if (row < nr) {
        hbuf[(row * 3 + 0) * TW + lane] = clamp255(a[q][0]);
        hbuf[(row * 3 + 1) * TW + lane] = clamp255(a[q][1]);
        hbuf[(row * 3 + 2) * TW + lane] = clamp255(a[q][2]);
      }
    }
    __syncthreads();
    // vertical pass: this chunk's share of the taps of output rows wave, wave + NW, ...
#pragma unroll
    for (int j = 0; j < RB / NW; ++j) {
      const int r = wave + NW * j;
      if (r < nrv) {
        const int lo = (vlo[r] > c0 ? vlo[r] : c0) - c0, hi = (vhi[r] < c0 + nr ? vhi[r] : c0 + nr) - c0;
        for (int jj = lo; jj < hi; ++jj) {
          const float wk = wv[r * CHT + jj];
          acc[j][0] = fmaf(wk, hbuf[(jj * 3 + 0) * TW + lane], acc[j][0]);
          acc[j][1] = fmaf(wk, hbuf[(jj * 3 + 1) * TW + lane], acc[j][1]);
          acc[j][2] = fmaf(wk, hbuf[(jj * 3 + 2) * TW + lane], acc[j][2]);
        }
      }
    }
    __syncthreads();
  }

  // the tile as it lies in the output: [row][channel][column], columns mirrored inside the tile when the sample is flipped
  const int ox0 = flip ? S - x0 - nx : x0, oc = flip ? nx - 1 - lane : lane;
  if (xv) {
#pragma unroll
    for (int j = 0; j < RB / NW; ++j) {
      const int r = wave + NW * j;
      if (r < nrv) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hbuf[(r * 3 + c) * TW + oc] = (clamp255(acc[j][c]) / 255.f - mean) / stdv;
      }
    }
  }
  __syncthreads();
  const int per_row = nx / PER;
  for (int e = tid; e < nrv * 3 * per_row; e += 256) {
    const int rc = e / per_row, q = e % per_row, r = rc / 3, c = rc % 3;
    const float* s = hbuf + rc * TW + q * PER;
    T* d = out + (((size_t)b * 3 + c) * S + y0 + r) * S + ox0 + q * PER;
    if constexpr (PER == 1) {
      d[0] = from_f<T>(s[0]);
    } else {
      float v[8];
      *(float4*)v = *(const float4*)s;
      if constexpr (PER == 8) *(float4*)(v + 4) = *(const float4*)(s + 4);
      if constexpr (PER == 8) Vec8<bf16>::store((bf16*)d, v);
      else *(float4*)d = *(const float4*)v;
    }
  }
}
}  // namespace

extern "C" int ldmae_crop_resize_flip_u8(const unsigned char* blob, long blob_bytes, const long* offset, const int* geom, void* out, int out_bf16,
                                         int B, int S, float mean, float stdev, void* stream) {
  LDMAE_REQUIRE(blob && offset && geom && out, "crop_resize_flip_u8: null pointer");
  LDMAE_REQUIRE(B >= 1 && S >= 1 && stdev != 0.f, "crop_resize_flip_u8: B=%d and S=%d must be positive and std non-zero", B, S);
  LDMAE_REQUIRE(S <= MAXN && blob_bytes >= 3, "crop_resize_flip_u8: S=%d above %d, or an empty blob (%ld bytes)", S, MAXN, blob_bytes);
  const long tiles = (long)cdiv(S, TW) * cdiv(S, RB) * B;
  LDMAE_REQUIRE(tiles < (1L << 31), "crop_resize_flip_u8: B=%d x S=%d needs %ld workgroups", B, S, tiles);
  const bool vec = S % (out_bf16 ? 8 : 4) == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid((unsigned)tiles), block(256);
  hipStream_t st = as_stream(stream);
  if (out_bf16) {
    if (vec) hipLaunchKernelGGL((crop_resize_flip_kernel<bf16, 8>), grid, block, 0, st, blob, blob_bytes, offset, geom, (bf16*)out, S, mean, stdev);
    else hipLaunchKernelGGL((crop_resize_flip_kernel<bf16, 1>), grid, block, 0, st, blob, blob_bytes, offset, geom, (bf16*)out, S, mean, stdev);
  } else {
    if (vec) hipLaunchKernelGGL((crop_resize_flip_kernel<float, 4>), grid, block, 0, st, blob, blob_bytes, offset, geom, (float*)out, S, mean, stdev);
    else hipLaunchKernelGGL((crop_resize_flip_kernel<float, 1>), grid, block, 0, st, blob, blob_bytes, offset, geom, (float*)out, S, mean, stdev);
  }
  LDMAE_CHECK_LAUNCH("crop_resize_flip_u8");
  return LDMAE_OK;
}
