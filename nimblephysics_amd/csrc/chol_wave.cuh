// Cholesky factorisation M = L L^T of the packed lower triangle of the
// joint-space mass matrix and the solves with it, one world per 64-lane
// wave (lane i = row i).  Used by the forward (ddq, impulses) and the
// backward (Minv products); stands in for the reference's articulated-body
// forward dynamics (dart/dynamics/Skeleton.cpp:13034) with the same result.
#pragma once
#include "spatial.cuh"
#include "wave.cuh"
#ifndef WAVE
#define WAVE 64
#endif

// In-place Cholesky of the packed lower triangle at A (row i at i(i+1)/2):
// left-looking (Crout) with one lane per row, one barrier per column.  The
// per-element subtraction order (k ascending) is that of the right-looking
// factorisation.  A column's scale is 1/L_jj from the hardware reciprocal
// square root refined by two Newton steps (L_jj = a_jj / sqrt(a_jj) =
// a_jj * rsq), so the column costs one multiply per lane instead of a square
// root and two divisions on its critical path (tools/micro/chol_bench.hip:
// 49.7k -> 39.5k clocks for n = 33; the factor differs from the divided one
// in the last bits only).
__device__ __forceinline__ double rsqrtRefined(double a) {
  double y = __builtin_amdgcn_rsq(a);
  y = y * (1.5 - 0.5 * a * y * y);
  return y * (1.5 - 0.5 * a * y * y);
}
__device__ __forceinline__ void choleskyLds(double* A, double* dinv, int n, int lane) {
  for (int j = 0; j < n; j++) {
    double sum = 0.0;
    if (lane >= j && lane < n) {
      const int ri = tri(lane, 0), rj = tri(j, 0);
      sum = A[ri + j];
      // blocks of 8: the sixteen loads issued before the multiply-adds
      int k = 0;
      for (; k + 8 <= j; k += 8) {
        double a[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { a[u] = A[ri + k + u]; c[u] = A[rj + k + u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) asm volatile("" : "+v"(a[u]), "+v"(c[u]));
#pragma unroll
        for (int u = 0; u < 8; u++) sum -= a[u] * c[u];
      }
      for (; k < j; k++) sum -= A[ri + k] * A[rj + k];
    }
    const double ajj = rdl(sum, j);
    const double y = rsqrtRefined(ajj);
    if (lane == j) { A[tri(j, j)] = ajj * y; dinv[j] = y; }
    else if (lane > j && lane < n) A[tri(lane, j)] = sum * y;
    WSYNC();
  }
}

// (A register-resident variant -- row i in VGPRs of lane i, row j broadcast
// through LDS per column -- measured 3x slower inside the forward kernel:
// fully unrolled it costs instruction-cache misses, and its rows spill when
// inlined.  The LDS form above is the one used.)
__device__ __forceinline__ void cholesky(double* A, double* dinv, int n, int lane) { choleskyLds(A, dinv, n, lane); }

// One substitution step of cholSolveReg for pivot row c (wave-uniform), l =
// this lane's L entry of the step: x_c <- x_c / L_cc on lane c, x_i <-
// fma(-L, x_c, x_i) on the lanes `upd`, every other lane keeps its value.
// Each lane forms its own x * (1 / L_ii); lane c keeps its product and
// broadcasts it: the same product as broadcasting x_c and multiplying by
// dinv[c].  The three cases are selects on values, so a step is
// straight-line code.
template <int K>
__device__ __forceinline__ void cholSolveStep(double (&x)[K], double l, double di, int c, bool at, bool upd) {
#pragma unroll
  for (int q = 0; q < K; q++) {
    const double p = x[q] * di;
    const double t = __builtin_fma(-l, rdl(p, c), x[q]);
    x[q] = at ? p : (upd ? t : x[q]);
  }
}

// Solve L L^T x = b for K right-hand sides at once, held in registers (row i
// on lane i): the K independent dependency chains interleave.  dinv[k] =
// 1 / L_kk; lane i loads dinv[i] once.  No branch and no exec-mask region
// inside a step (cholSolveStep), and the steps go in blocks of FB (forward
// substitution) and BB (backward) whose L entries are loaded together, ahead
// of the block's readlane -> FMA chain.  All loads are unconditional and stay
// inside the packed triangle; what a lane reads beyond its own part of a
// column or row is selected away:
//   forward: lane i reads its row, Lm[tri(i, 0) + k] for every k < n; for
//     i <= n - 2 the last of them, tri(i, 0) + n - 1, is at most tri(n - 1, 0),
//     and lanes >= n read row n - 1;
//   backward: row k is contiguous, lane i reads Lm[tri(k, 0) + min(i, k)].
// Lanes >= n return their x unchanged.  Per element the roundings are those
// of the plain substitution: k ascending, x_k <- x_k dinv_k, x_i <-
// fma(-L_ik, x_k, x_i) for i > k; then the mirror image with L^T.
template <int K, int FB, int BB>
__device__ __forceinline__ void cholSolveRegBlocked(const double* Lm, const double* dinv, double (&x)[K], int n,
                                                    int lane) {
  if (n <= 0) return;
  const bool in = lane < n;
  const int li = in ? lane : n - 1;
  const double di = dinv[li];
  const double* row = Lm + tri(li, 0);
  int k = 0;
  for (; k + FB <= n; k += FB) {
    double l[FB];
#pragma unroll
    for (int u = 0; u < FB; u++) l[u] = row[k + u];
#pragma unroll
    for (int u = 0; u < FB; u++) asm volatile("" : "+v"(l[u]));
#pragma unroll
    for (int u = 0; u < FB; u++) cholSolveStep<K>(x, l[u], di, k + u, lane == k + u, in && lane > k + u);
  }
  for (; k < n; k++) cholSolveStep<K>(x, row[k], di, k, lane == k, in && lane > k);
  k = n - 1;
  for (; k - BB + 1 >= 0; k -= BB) {
    double l[BB];
#pragma unroll
    for (int u = 0; u < BB; u++) l[u] = Lm[tri(k - u, 0) + (lane < k - u ? lane : k - u)];
#pragma unroll
    for (int u = 0; u < BB; u++) asm volatile("" : "+v"(l[u]));
#pragma unroll
    for (int u = 0; u < BB; u++) cholSolveStep<K>(x, l[u], di, k - u, lane == k - u, lane < k - u);
  }
  for (; k >= 0; k--) cholSolveStep<K>(x, Lm[tri(k, 0) + (lane < k ? lane : k)], di, k, lane == k, lane < k);
}
// (Block sizes: tools/micro/chol_solve_bench.hip.)
template <int K>
__device__ __forceinline__ void cholSolveReg(const double* Lm, const double* dinv, double (&x)[K], int n, int lane) {
  cholSolveRegBlocked<K, 8, 8>(Lm, dinv, x, n, lane);
}

// The same solve with an if / else per case and the two LDS loads inside the
// step: about a dozen exec-mask branches per step once compiled, two to three
// times the clocks of the form above (chol_solve_bench.hip's `branchy`).
// Same roundings per element.  Kept for the forward kernels' ddq solve only:
// there the select form halves the stage (19.5k -> 9.4k clocks) without
// shortening the kernel, because the world's wave then waits that much longer
// for the helper wave's Y = L^-1 J^T, and at the 256-VGPR cap it makes two
// mesh instances spill more (profiles/chol_solve/).  (Loading eight steps' L
// entries ahead in *this* form measured slower, 19.8k -> 22.7k clocks for the
// 33-dof unconstrained solve: the LDS latency is the smaller part of its
// step.)
template <int K>
__device__ __forceinline__ void cholSolveRegBranchy(const double* Lm, const double* dinv, double (&x)[K], int n,
                                                    int lane) {
  for (int k = 0; k < n; k++) {
    const double dk = dinv[k];
    const double lk = (lane > k && lane < n) ? Lm[tri(lane, k)] : 0.0;
#pragma unroll
    for (int q = 0; q < K; q++) {
      const double xk = rdl(x[q], k) * dk;
      if (lane == k) x[q] = xk;
      else if (lane > k) x[q] -= lk * xk;
    }
  }
  for (int k = n - 1; k >= 0; k--) {
    const double dk = dinv[k];
    const double lk = lane < k ? Lm[tri(k, lane)] : 0.0;
#pragma unroll
    for (int q = 0; q < K; q++) {
      const double xk = rdl(x[q], k) * dk;
      if (lane == k) x[q] = xk;
      else if (lane < k) x[q] -= lk * xk;
    }
  }
}

template <bool kBranchy = false>
__device__ __forceinline__ void cholSolve(const double* Lm, const double* dinv, double* x, int n, int lane) {
  double xr[1] = {lane < n ? x[lane] : 0.0};
  if constexpr (kBranchy) cholSolveRegBranchy<1>(Lm, dinv, xr, n, lane);
  else cholSolveReg<1>(Lm, dinv, xr, n, lane);
  WSYNC();
  if (lane < n) x[lane] = xr[0];
  WSYNC();
}
