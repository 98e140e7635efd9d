// Worst error of the device math functions the elementwise kernels call, each ALONE against the f64 host function of the same f32 argument,
// over the argument ranges the layer tests use (tests/layer_check.py takes its measured constants from this program's output).
// Errors are printed in units of u = 2^-24: relative (|y - r| / |r| / u, where r is a normal f32) and absolute (|y - r| / u).
//   make probe && probe/intrinsic_probe
#include "../common.h"
#include <cmath>
#include <cstdio>
#include <vector>

enum Fn { EXP2, FEXP, EXPF, LOGF, COSF, SINF, ERFF, RCP, ERFAS, TANHX, FSIG, NFN };
static const char* NAMES[NFN] = {"exp2 (v_exp)", "__expf", "expf", "logf", "cosf", "sinf", "erff", "rcp (v_rcp)", "erf_as", "tanh_exp", "fast_sigmoid"};

__device__ __forceinline__ float tanh_exp_p(float u) { return 1.f - 2.f / (__expf(2.f * u) + 1.f); }      // csrc/vmae.hip tanh_exp
template <int F> __device__ __forceinline__ float apply(float x) {
  if (F == EXP2) return __builtin_amdgcn_exp2f(x);
  if (F == FEXP) return __expf(x);
  if (F == EXPF) return expf(x);
  if (F == LOGF) return logf(x);
  if (F == COSF) return cosf(x);
  if (F == SINF) return sinf(x);
  if (F == ERFF) return erff(x);
  if (F == RCP) return __builtin_amdgcn_rcpf(x);
  if (F == ERFAS) return erf_as(x);
  if (F == TANHX) return tanh_exp_p(x);
  return fast_sigmoid(x);
}
template <int F> __global__ void eval_kernel(const float* __restrict__ x, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = apply<F>(x[i]);
}
static double ref(int f, double x) {
  switch (f) {
    case EXP2: return exp2(x);
    case FEXP: case EXPF: return exp(x);
    case LOGF: return log(x);
    case COSF: return cos(x);
    case SINF: return sin(x);
    case ERFF: case ERFAS: return erf(x);
    case RCP: return 1.0 / x;
    case TANHX: return tanh(x);
    default: return 1.0 / (1.0 + exp(-x));
  }
}
template <int F> static void launch(const float* x, float* y, int n) { hipLaunchKernelGGL(eval_kernel<F>, dim3((n + 255) / 256), dim3(256), 0, 0, x, y, n); }

// n arguments in [lo, hi]: half uniform, half with log-spaced magnitudes down to `tiny` (both signs where the range has both), plus the ends and 0
static std::vector<float> grid(double lo, double hi, double tiny, int n) {
  std::vector<float> v;
  v.reserve(n + 8);
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
  for (int i = 0; i < n / 2; ++i) v.push_back((float)(lo + (hi - lo) * rnd()));
  const double top = fmax(fabs(lo), fabs(hi));
  for (int i = 0; i < n / 2; ++i) {
    double m = tiny * pow(top / tiny, rnd());
    if (lo < 0 && (hi <= 0 || rnd() < 0.5)) m = -m;
    if (m >= lo && m <= hi) v.push_back((float)m);
  }
  v.push_back((float)lo); v.push_back((float)hi);
  if (lo <= 0 && hi >= 0) { v.push_back(0.f); v.push_back(-0.f); }
  return v;
}

int main() {
  struct Job { int f; double lo, hi, tiny; } jobs[] = {
    {EXP2, -126, 127.99, 1e-30}, {FEXP, -87, 88, 1e-30}, {EXPF, -87, 88, 1e-30}, {EXPF, -15, 10, 1e-30}, {LOGF, 1, 1e5, 1}, {COSF, 0, 1000, 1e-30}, {SINF, 0, 1000, 1e-30},
    {ERFF, -8.5, 8.5, 1e-30}, {RCP, 1, 1e30, 1}, {RCP, 1, 4, 1}, {ERFAS, -8.5, 8.5, 1e-30}, {TANHX, -72, 72, 1e-30}, {FSIG, -87, 87, 1e-30}};
  const int n = 1 << 22;
  float *dx, *dy;
  if (hipMalloc(&dx, (n + 8) * 4) != hipSuccess || hipMalloc(&dy, (n + 8) * 4) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  const double u = ldexp(1.0, -24), tiny32 = ldexp(1.0, -126);
  for (const Job& j : jobs) {
    std::vector<float> x = grid(j.lo, j.hi, j.tiny, n), y(x.size());
    const int m = (int)x.size();
    hipMemcpy(dx, x.data(), m * 4, hipMemcpyHostToDevice);
    switch (j.f) {
      case EXP2: launch<EXP2>(dx, dy, m); break;   case FEXP: launch<FEXP>(dx, dy, m); break;   case EXPF: launch<EXPF>(dx, dy, m); break;
      case LOGF: launch<LOGF>(dx, dy, m); break;   case COSF: launch<COSF>(dx, dy, m); break;   case SINF: launch<SINF>(dx, dy, m); break;
      case ERFF: launch<ERFF>(dx, dy, m); break;   case RCP: launch<RCP>(dx, dy, m); break;     case ERFAS: launch<ERFAS>(dx, dy, m); break;
      case TANHX: launch<TANHX>(dx, dy, m); break; default: launch<FSIG>(dx, dy, m); break;
    }
    if (hipMemcpy(y.data(), dy, m * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: the kernel failed\n", NAMES[j.f]); return 1; }
    double mrel = 0, mabs = 0, mexcess = -1e30, arel = 0, aabs = 0;
    int bad = 0;
    for (int i = 0; i < m; ++i) {
      const double r = ref(j.f, (double)x[i]), e = fabs((double)y[i] - r);
      if (!std::isfinite(y[i])) { ++bad; continue; }
      if (e / u > mabs) { mabs = e / u; aabs = x[i]; }
      if (fabs(r) >= tiny32) {
        const double rel = e / fabs(r) / u;
        if (rel > mrel) { mrel = rel; arel = x[i]; }
        if (rel - 2 * fabs((double)x[i]) > mexcess) mexcess = rel - 2 * fabs((double)x[i]);
      }
    }
    printf("%-14s [%g, %g] n=%d  max rel %.3f u (at %.9g)  max abs %.3f u (at %.9g)  max (rel - 2|x|) %.3f u  non-finite %d\n", NAMES[j.f], j.lo, j.hi, m, mrel, arel, mabs,
           aabs, mexcess, bad);
  }
  hipFree(dx); hipFree(dy);
  return 0;
}
