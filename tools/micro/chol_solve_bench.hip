// The solves with the Cholesky factor of the 33 x 33 joint-space mass matrix
// (csrc/chol_wave.cuh, cholSolveReg<K>), one world per 64-lane wave, one wave
// per workgroup, 1024 worlds, 40 KB LDS per workgroup as in the forward kernel:
//   branchy    : cholSolveRegBranchy, the form used before -- an if / else
//                per case and per right-hand side, the two LDS loads inside
//                the step
//   select_8_8 : the product's form: selects on values, blocks of 8 steps in
//                both substitutions
//   select_4_4 : blocks of 4
//   select_8_1 : forward substitution in blocks of 8, backward step by step
//   select_1_1 : selects, no blocks
//   zeroed_8_8 : blocks of 8, a zeroed L entry instead of the select on the
//                updated value (NOT the same bits in general: fma(-0, x_k, x)
//                turns x = -0.0 into +0.0 and lets a non-finite x_k reach
//                lanes the select leaves alone; timed for comparison only)
// for K = 1, 2, 4, 5 right-hand sides.  Prints JSON: mean and max clocks per
// solve over the worlds, clocks per substitution step (2 n steps per solve)
// and whether the results equal `branchy` bit for bit.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../nimblephysics_amd/csrc/chol_wave.cuh"

#define REPS 40
#define NDOF 33
#define NVAR 6

template <int K>
__device__ __forceinline__ void zeroedStep(double (&x)[K], double l, double di, int c, bool at, bool upd) {
  const double lz = upd ? l : 0.0;
#pragma unroll
  for (int q = 0; q < K; q++) {
    const double p = x[q] * di;
    const double t = __builtin_fma(-lz, rdl(p, c), x[q]);
    x[q] = at ? p : t;
  }
}
template <int K>
__device__ __forceinline__ void solveZeroed(const double* Lm, const double* dinv, double (&x)[K], int n, int lane) {
  if (n <= 0) return;
  const bool in = lane < n;
  const int li = in ? lane : n - 1;
  const double di = dinv[li];
  const double* row = Lm + tri(li, 0);
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double l[8];
#pragma unroll
    for (int u = 0; u < 8; u++) l[u] = row[k + u];
#pragma unroll
    for (int u = 0; u < 8; u++) asm volatile("" : "+v"(l[u]));
#pragma unroll
    for (int u = 0; u < 8; u++) zeroedStep<K>(x, l[u], di, k + u, lane == k + u, in && lane > k + u);
  }
  for (; k < n; k++) zeroedStep<K>(x, row[k], di, k, lane == k, in && lane > k);
  k = n - 1;
  for (; k - 7 >= 0; k -= 8) {
    double l[8];
#pragma unroll
    for (int u = 0; u < 8; u++) l[u] = Lm[tri(k - u, 0) + (lane < k - u ? lane : k - u)];
#pragma unroll
    for (int u = 0; u < 8; u++) asm volatile("" : "+v"(l[u]));
#pragma unroll
    for (int u = 0; u < 8; u++) zeroedStep<K>(x, l[u], di, k - u, lane == k - u, lane < k - u);
  }
  for (; k >= 0; k--) zeroedStep<K>(x, Lm[tri(k, 0) + (lane < k ? lane : k)], di, k, lane == k, lane < k);
}

// Lg [W, P], dg [W, n], xg [W, K, 64] -> out [W, K, 64], clk [W]
template <int V, int K>
__global__ void __launch_bounds__(64) bench(const double* __restrict__ Lg, const double* __restrict__ dg,
                                            const double* __restrict__ xg, double* __restrict__ out,
                                            long long* __restrict__ clk) {
  extern __shared__ double smem[];
  double* Lm = smem;
  double* dinv = smem + 600;
  const int lane = threadIdx.x;
  // n a run-time value, as in the kernels (clk arrives zeroed)
  const int n = uni(NDOF + (int)clk[blockIdx.x]), P = NDOF * (NDOF + 1) / 2;
  for (int t = lane; t < P; t += 64) Lm[t] = Lg[(size_t)blockIdx.x * P + t];
  if (lane < NDOF) dinv[lane] = dg[(size_t)blockIdx.x * NDOF + lane];
  WSYNC();
  long long tot = 0;
  double x[K];
  for (int r = 0; r < REPS; r++) {
#pragma unroll
    for (int q = 0; q < K; q++) x[q] = xg[((size_t)blockIdx.x * K + q) * 64 + lane];
#pragma unroll
    for (int q = 0; q < K; q++) asm volatile("" : "+v"(x[q]));
    const long long t0 = __builtin_amdgcn_s_memtime();
    if constexpr (V == 0) cholSolveRegBranchy<K>(Lm, dinv, x, n, lane);
    else if constexpr (V == 1) cholSolveRegBlocked<K, 8, 8>(Lm, dinv, x, n, lane);
    else if constexpr (V == 2) cholSolveRegBlocked<K, 4, 4>(Lm, dinv, x, n, lane);
    else if constexpr (V == 3) cholSolveRegBlocked<K, 8, 1>(Lm, dinv, x, n, lane);
    else if constexpr (V == 4) cholSolveRegBlocked<K, 1, 1>(Lm, dinv, x, n, lane);
    else solveZeroed<K>(Lm, dinv, x, n, lane);
#pragma unroll
    for (int q = 0; q < K; q++) asm volatile("" : "+v"(x[q]));
    const long long t1 = __builtin_amdgcn_s_memtime();
    tot += t1 - t0;
  }
#pragma unroll
  for (int q = 0; q < K; q++) out[((size_t)blockIdx.x * K + q) * 64 + lane] = x[q];
  if (lane == 0) clk[blockIdx.x] = tot / REPS;
}

static const int W = 1024;
static double *dL, *dD, *dX;

template <int V, int K>
static bool run(std::vector<double>& res, double& mean, double& mx) {
  double* dO;
  long long* dC;
  const size_t nx = (size_t)W * K * 64;
  if (hipMalloc(&dO, nx * 8) != hipSuccess || hipMalloc(&dC, W * 8) != hipSuccess) return false;
  (void)hipMemset(dC, 0, W * 8);
  hipLaunchKernelGGL((bench<V, K>), dim3(W), dim3(64), 40 * 1024, 0, dL, dD, dX, dO, dC);
  if (hipDeviceSynchronize() != hipSuccess) return false;
  res.resize(nx);
  std::vector<long long> C(W);
  (void)hipMemcpy(res.data(), dO, nx * 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(C.data(), dC, W * 8, hipMemcpyDeviceToHost);
  mean = 0;
  mx = 0;
  for (auto c : C) { mean += (double)c / W; mx = fmax(mx, (double)c); }
  (void)hipFree(dO);
  (void)hipFree(dC);
  return true;
}

template <int K>
static bool runK(bool first) {
  const char* nm[NVAR] = {"branchy", "select_8_8", "select_4_4", "select_8_1", "select_1_1", "zeroed_8_8"};
  std::vector<double> res[NVAR];
  double mean[NVAR], mx[NVAR];
  if (!run<0, K>(res[0], mean[0], mx[0]) || !run<1, K>(res[1], mean[1], mx[1]) || !run<2, K>(res[2], mean[2], mx[2]) ||
      !run<3, K>(res[3], mean[3], mx[3]) || !run<4, K>(res[4], mean[4], mx[4]) || !run<5, K>(res[5], mean[5], mx[5]))
    return false;
  std::printf("%s\"K%d\": {", first ? "" : ", ", K);
  for (int v = 0; v < NVAR; v++) {
    const bool same = std::memcmp(res[v].data(), res[0].data(), res[0].size() * 8) == 0;
    std::printf("%s\"%s\": {\"clk_mean\": %.0f, \"clk_max\": %.0f, \"clk_per_step\": %.1f, \"bits_equal_branchy\": %s}",
                v ? ", " : "", nm[v], mean[v], mx[v], mean[v] / (2 * NDOF), same ? "true" : "false");
  }
  std::printf("}");
  return true;
}

int main() {
  const int n = NDOF, P = n * (n + 1) / 2;
  std::vector<double> L((size_t)W * P), D((size_t)W * n), X((size_t)W * 5 * 64, 0.0);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1103515245u + 12345u; return ((s >> 8) & 0xFFFFFF) / 16777216.0 - 0.5; };
  for (int w = 0; w < W; w++) {
    std::vector<double> B(n * n), F(n * n, 0.0);
    for (auto& v : B) v = rnd();
    for (int i = 0; i < n; i++)
      for (int j = 0; j <= i; j++) {
        double acc = i == j ? n : 0.0;
        for (int k = 0; k < n; k++) acc += B[i * n + k] * B[j * n + k];
        F[i * n + j] = acc;
      }
    for (int j = 0; j < n; j++) {  // host Cholesky, lower triangle in place
      for (int k = 0; k < j; k++)
        for (int i = j; i < n; i++) F[i * n + j] -= F[i * n + k] * F[j * n + k];
      const double d = std::sqrt(F[j * n + j]);
      for (int i = j; i < n; i++) F[i * n + j] /= d;
    }
    for (int i = 0; i < n; i++) {
      for (int k = 0; k <= i; k++) L[(size_t)w * P + i * (i + 1) / 2 + k] = F[i * n + k];
      D[(size_t)w * n + i] = 1.0 / F[i * n + i];
    }
  }
  // the K = 5 layout [W, 5, 64] read with the kernel's own K: any K sees
  // random right-hand sides on lanes < n and zeros above
  for (size_t t = 0; t < X.size(); t++)
    if ((int)(t % 64) < n) X[t] = rnd();
  if (hipMalloc(&dL, L.size() * 8) != hipSuccess || hipMalloc(&dD, D.size() * 8) != hipSuccess ||
      hipMalloc(&dX, X.size() * 8) != hipSuccess)
    return 1;
  (void)hipMemcpy(dL, L.data(), L.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(dD, D.data(), D.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(dX, X.data(), X.size() * 8, hipMemcpyHostToDevice);
  std::printf("{\"n\": %d, \"worlds\": %d, \"steps_per_solve\": %d, ", n, W, 2 * n);
  if (!runK<1>(true) || !runK<2>(false) || !runK<4>(false) || !runK<5>(false)) {
    std::printf("\n");
    std::fprintf(stderr, "a launch failed\n");
    return 1;
  }
  std::printf("}\n");
  return 0;
}
