// The body of the RMSNorm + modulate forward row kernels, written once: rmsnorm_mod_fwd_kernel (elementwise.hip) stores the modulated row,
// rmsnorm_mod_fwd_mx8_kernel (mx8.hip) quantises it, and the two are pinned to each other bitwise.  Included between the braces of a kernel
// that has the parameters x, w, shift, scale, mod_ld, rstd, M, D, rpb, eps, center and the template parameters NCH, FULL, and that defines
//   NORM_EMIT(m, a, b, y)    what becomes of the four modulated values y of row m at columns (a) + (b) .. + 3
// (the FULL form passes a = 4 * lane, b = 256 * i; the guarded form a = 4 * c, b = 0).  The hook takes the offset in two parts so that the
// store keeps the pointer association `out + m * D + a + b` of the kernel it was lifted from.
// This is included text and not a __device__ function ON PURPOSE: a helper is optimised before it is inlined, and with the store passed
// as a lambda the packed multiply / fma sequence of the sum of squares changed (rmsnorm_mod_fwd_kernel<1, bf16, FULL>) -- the result bits
// are those contraction choices.  As text, every kernel compiles to the instructions it had with its own copy.
//
// center (guarded form only): LayerNorm WITHOUT affine parameters (the use_rmsnorm=False blocks, lightningdit.py:200-201) = the RMS norm of
// the centred row, w = NULL -> 1: y = (x - mean) * rsqrt(mean((x - mean)^2) + eps) * (1 + scale) + shift
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = D >> 2;
  float4 wv[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) { const int c = lane + 64 * i; wv[i] = c < nch ? (w ? *(const float4*)(w + 4 * c) : f4(1.f)) : f4(0.f); }
  if constexpr (FULL) {
    const int m0 = (blockIdx.x * 4 + wave) * 4, b = m0 / rpb;
    float4 sc1[NCH], sh[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      sc1[i] = scale ? f4(1.f) + *(const float4*)(scale + (size_t)b * mod_ld + 4 * lane + 256 * i) : f4(1.f);
      sh[i] = shift ? *(const float4*)(shift + (size_t)b * mod_ld + 4 * lane + 256 * i) : f4(0.f);
    }
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + r;
      float4 xv[NCH];
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) xv[i] = *(const float4*)(x + (size_t)m * D + 4 * lane + 256 * i);
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
        NORM_EMIT(m, 4 * lane, 256 * i, y);
      }
    }
    return;
  }
  for (int r = 0; r < 4; ++r) {
    const int m = (blockIdx.x * 4 + wave) * 4 + r;
    if (m >= M) return;
    const int b = m / rpb;
    float4 xv[NCH];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      xv[i] = c < nch ? *(const float4*)(x + (size_t)m * D + 4 * c) : f4(0.f);
      ss += hsum(xv[i] * xv[i]);
    }
    if (center) {
      float s1 = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) s1 += hsum(xv[i]);
      const float mean = wave_sum(s1) / (float)D;
      ss = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        if (lane + 64 * i < nch) xv[i] = xv[i] - f4(mean);
        ss += hsum(xv[i] * xv[i]);
      }
    }
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
        NORM_EMIT(m, 4 * c, 0, y);
      }
    }
  }
