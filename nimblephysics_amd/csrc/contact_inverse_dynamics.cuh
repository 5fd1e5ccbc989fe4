// Batched contact inverse dynamics: the joint torques and the wrenches on k
// named contact bodies that produce a given motion of a floating-base skeleton
// whose six root dofs are not actuated -- the reference's
// Skeleton::getContactInverseDynamics (dart/dynamics/Skeleton.cpp:9449, k = 1)
// and Skeleton::getMultipleContactInverseDynamics (:9578), for a batch.
//
//   tau_full = M a + C - tau_ext + D v + K (q - q0 + dt v)     (invDynWorld)
//   r        = tau_full[r0 .. r0+5]                     the root's residual
//   Jr       = [Jr_1; ..; Jr_k],  Jr_i[:, c] = Ad_{Tw_i^-1} Sw[r0 + c]
//              (6k x 6: the body-frame Jacobians' root columns; the
//              reference's jacBlock is Jr^T)
//   N = Jr^T diag(w) Jr,  y = N^-1 (r - Jr^T F0),  F = F0 + diag(w) Jr y
//   tau      = tau_full - J^T F,  exactly 0 in the root rows
//
// With guesses F0 the weights are 1: the F nearest F0 with Jr^T F = r, the
// reference's KKT system (:9652-9664).  Without, F0 = 0 and w = 1 on the
// torque and 100 on the force components: the reference's B^-1 of eps = 0.01
// (:9643-9650), the solution with the smallest moments (its min-norm solve
// :9677).  Both closed forms rest on Jr^T having full row rank, which it has:
// every Jr_i is an invertible adjoint, so N is SPD.
//
// One world per 64-lane workgroup, no helper wave, included by timestep.hip
// like inverse_dynamics.cuh.  The LDS is the inverse-dynamics forward's layout
// (capi.cpp invDynLayout) with this kernel's own areas behind it; their
// offsets, k, r0 and the bodies come in ContactIdArgs (model.h), by value.
// kPW and kExt are always set, as in inverse_dynamics.cuh.
#pragma once

// Contact body i (lane-dependent) of the packed list.
__device__ __forceinline__ int contactBody(const ContactIdArgs& P, int i) {
  return (int)((P.bodies >> (8 * i)) & 0xffull);
}

__device__ __forceinline__ void contactInvDynWorld(const ModelDev* __restrict__ mdp, const Layout& L,
                                                   const ContactIdArgs& P, const double* __restrict__ state,
                                                   const double* __restrict__ ddq,
                                                   const double* __restrict__ bodyInertia, int inertiaStride,
                                                   const double* __restrict__ bodyWrench, int wrenchStride,
                                                   int wrenchFrame, const double* __restrict__ guesses,
                                                   double* __restrict__ tau, double* __restrict__ contactWrenches) {
  extern __shared__ double s[];
  const ModelDev& md = *mdp;
  const int lane = threadIdx.x;
  const int n = md.n;
  const int env = blockIdx.x;
  const int k = P.k, rows = 6 * P.k, r0 = P.r0;
  {
    const double* st = state + (size_t)env * 2 * n;
    const double* a = ddq + (size_t)env * n;
    for (int i = lane; i < n; i += WAVE) {
      s[L.q + i] = st[i];
      s[L.v + i] = st[n + i];
      s[L.x + i] = a[i];
    }
    for (int i = lane; i < 6 * md.nb; i += WAVE) s[P.E + i] = 0.0;
    WSYNC();
  }
  // 1. tau_full, as invDynWorld, kept in LDS (L.rhs)
  kinematics(md, s, L, lane, s + L.x);
  composites<true, true>(md, s, L, lane, bodyInertia + (size_t)env * inertiaStride,
                         bodyWrench + (size_t)env * wrenchStride, wrenchFrame);
  massMatrixAndBias(md, s, L, lane, s + L.rhs);
  for (int i = lane; i < n; i += WAVE) {
    const double qi = s[L.q + i], vi = s[L.v + i];
    const double springF = md.spring[i] * (qi - md.rest[i] + vi * md.dt);
    const double dampF = md.damping[i] * vi;
    s[L.rhs + i] = s[L.rhs + i] + dampF + springF;
  }
  // 2. Jr: lane = (body i, root column c)
  if (lane < rows) {
    const int i = lane / 6, c = lane - 6 * i;
    double col[6];
    twistInWrenchFrame(s + L.Sw + 6 * (r0 + c), NIMBLE_WRENCH_BODY, s + L.Tw + 12 * contactBody(P, i), col);
#pragma unroll
    for (int r = 0; r < 6; r++) s[P.Jr + 6 * (6 * i + r) + c] = col[r];
  }
  WSYNC();
  // 3. the 21 packed entries of N on lanes 0 .. 20, the right-hand side
  // r - Jr^T F0 on lanes 32 .. 37
  const double wForce = guesses != nullptr ? 1.0 : 100.0;
  const double* F0 = guesses != nullptr ? guesses + (size_t)env * rows : nullptr;
  if (lane < 21) {
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= lane) j++;
    const int c = lane - j * (j + 1) / 2;
    double sum = 0.0;
    for (int i = 0; i < k; i++) {
      const double* Ji = s + P.Jr + 36 * i;
#pragma unroll
      for (int r = 0; r < 6; r++) sum += (r < 3 ? 1.0 : wForce) * Ji[6 * r + j] * Ji[6 * r + c];
    }
    s[P.N + tri(j, c)] = sum;
  } else if (lane >= 32 && lane < 38) {
    const int c = lane - 32;
    double sum = s[L.rhs + r0 + c];
    if (F0 != nullptr)
      for (int m = 0; m < rows; m++) sum -= s[P.Jr + 6 * m + c] * F0[m];
    s[P.y + c] = sum;
  }
  WSYNC();
  // 4. N y = rhs
  cholesky(s + P.N, s + P.dinv, 6, lane);
  cholSolve(s + P.N, s + P.dinv, s + P.y, 6, lane);
  // 5. F = F0 + diag(w) Jr y, lane = row of F
  if (lane < rows) {
    const int i = lane / 6, r = lane - 6 * i;
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) sum += s[P.Jr + 6 * lane + c] * s[P.y + c];
    const double f = (F0 != nullptr ? F0[lane] : 0.0) + (r < 3 ? 1.0 : wForce) * sum;
    s[P.Fc + lane] = f;
    contactWrenches[(size_t)env * rows + lane] = f;
  }
  WSYNC();
  // 6. E_i = the world-frame wrench of F_i at its body, summed up the tree as
  // in invDynBodyForces; tau = tau_full - S . E
  if (lane < k) {
    const int b = contactBody(P, lane);
    worldWrench(s + P.Fc + 6 * lane, NIMBLE_WRENCH_BODY, s + L.Tw + 12 * b, s + P.E + 6 * b);
  }
  WSYNC();
  if (lane < 6) {
    const int off = P.E + lane;
#pragma unroll 4
    for (int e = 0; e < md.numAcc; e++) {
      const int p = md.accEdge[e][0], c = md.accEdge[e][1];
      s[off + 6 * p] += s[off + 6 * c];
    }
  }
  WSYNC();
  const int rootSkel = md.skel[md.dofBody[r0]];
  for (int j = lane; j < n; j += WAVE) {
    const int b = md.dofBody[j];
    const double full = s[L.rhs + j];
    double t = full - dot6(s + L.Sw + 6 * j, s + P.E + 6 * b);
    // the dofs of other skeletons keep tau_full; the root is not actuated
    if (md.skel[b] != rootSkel) t = full;
    if (j >= r0 && j < r0 + 6) t = 0.0;
    tau[(size_t)env * n + j] = t;
  }
}

extern "C" __global__ void __launch_bounds__(WAVE)
nimble_contact_inverse_dynamics_kernel(const ModelDev* __restrict__ mdp, Layout L, ContactIdArgs P,
                                       const double* __restrict__ state, const double* __restrict__ ddq,
                                       const double* __restrict__ bodyInertia, int inertiaStride,
                                       const double* __restrict__ bodyWrench, int wrenchStride, int wrenchFrame,
                                       const double* __restrict__ guesses, double* __restrict__ tau,
                                       double* __restrict__ contactWrenches) {
  contactInvDynWorld(mdp, L, P, state, ddq, bodyInertia, inertiaStride, bodyWrench, wrenchStride, wrenchFrame,
                     guesses, tau, contactWrenches);
}
