// Batched differentiable inverse dynamics, mass matrix and bias forces.
//
//   tau = ID(q, v, a) = M(q) a + C(q, v) - tau_ext(q) + D v + K (q - q0 + dt v)
//
// -- the reference's Skeleton::getInverseDynamics (dart/dynamics/Skeleton.cpp:9433:
// multiplyByImplicitMassMatrix :11124, getDampingForce :11355, getSpringForce
// :11388, - getExternalForces()) over all of the world's dofs, in this
// project's conventions: the exact inverse of the contact-free step,
// timestep(world, (q, v), tau) has v' = v + dt a.  C holds gravity, tau_ext is
// the generalized force of body_wrench (wrench.cuh), contacts play no part.
//
// Two kernels, one world per 64-lane workgroup, included by timestep.hip for
// the functions they share with the step (kinematics with ddq = a,
// composites, massMatrixAndBias, adjointVectors): they run those pieces and
// nothing else -- no Cholesky, no solves, no contact pool, no snapshot, no
// helper wave -- each on a lean LDS layout of its own (capi.cpp
// invDynLayout), passed as a kernel argument.  kPW and kExt are always set:
// the model's own parameters come as one [nb][10] block with batch stride 0,
// absent wrenches as one zero [nb][6] block with batch stride 0 (every world
// reads the same cached lines).
//
// The inertial parameters (inertia_grad.cuh): the backward's kInertia
// instance, nimble_inverse_dynamics_backward_inertia_kernel, adds gradInertia
// = (d tau / d theta)^T g, and nimble_inverse_dynamics_inertia_jacobian_kernel
// writes the matrix d tau / d theta itself.
#pragma once

#include "inertia_grad.cuh"

// Body forces without the wrench at the accelerations in L.A, summed over the
// subtrees into L.F: f_b = I_b (A_b - a_g) + V_b x* (I_b V_b), the forces of
// composites<true>() without its composite inertias (which the caller has
// finished with, and which are not formed again).
__device__ __forceinline__ void invDynBodyForces(const ModelDev& md, double* s, const Layout& L, int lane,
                                                 const double* bi) {
  const double ag[6] = {0, 0, 0, md.g[0], md.g[1], md.g[2]};
  if (lane < md.nb) {
    const int b = lane;
    double I[36];
    worldInertia<true>(md, bi, s + L.Tw + 12 * b, b, I);
    double u[6], h[6], f[6], vxh[6];
    for (int i = 0; i < 6; i++) u[i] = s[L.A + 6 * b + i] - ag[i];
    mv6(I, u, f);
    mv6(I, s + L.V + 6 * b, h);
    crf(s + L.V + 6 * b, h, vxh);
    for (int i = 0; i < 6; i++) s[L.F + 6 * b + i] = f[i] + vxh[i];
  }
  WSYNC();
  if (lane < 6) {
    const int off = L.F + lane;
#pragma unroll 4
    for (int k = 0; k < md.numAcc; k++) {
      const int p = md.accEdge[k][0], c = md.accEdge[k][1];
      s[off + 6 * p] += s[off + 6 * c];
    }
  }
  WSYNC();
}

// tau [B][n]; massMatrix [B][n][n] (full symmetric: World::getMassMatrix,
// dart/simulation/World.cpp:1974) and bias [B][n] (C(q, v) with gravity,
// without damping, spring or wrench: World::getCoriolisAndGravityForces,
// World.cpp:1943) when not nullptr.
__device__ __forceinline__ void invDynWorld(const ModelDev* __restrict__ mdp, const Layout& L,
                                            const double* __restrict__ state, const double* __restrict__ ddq,
                                            const double* __restrict__ bodyInertia, int inertiaStride,
                                            const double* __restrict__ bodyWrench, int wrenchStride,
                                            int wrenchFrame, double* __restrict__ tau,
                                            double* __restrict__ massMatrix, double* __restrict__ bias) {
  extern __shared__ double s[];
  const ModelDev& md = *mdp;
  const int lane = threadIdx.x;
  const int n = md.n;
  const int env = blockIdx.x;
  {
    const double* st = state + (size_t)env * 2 * n;
    const double* a = ddq + (size_t)env * n;
    for (int i = lane; i < n; i += WAVE) {
      s[L.q + i] = st[i];
      s[L.v + i] = st[n + i];
      s[L.x + i] = a[i];
    }
    WSYNC();
  }
  const double* bi = bodyInertia + (size_t)env * inertiaStride;
  // A = the accelerations at ddq = a, so the bias of the recursion is
  // M a + C - tau_ext (Skeleton::getInverseDynamics runs the same recursion)
  kinematics(md, s, L, lane, s + L.x);
  composites<true, true>(md, s, L, lane, bi, bodyWrench + (size_t)env * wrenchStride, wrenchFrame);
  massMatrixAndBias(md, s, L, lane, s + L.rhs);
  for (int i = lane; i < n; i += WAVE) {
    const double qi = s[L.q + i], vi = s[L.v + i];
    const double springF = md.spring[i] * (qi - md.rest[i] + vi * md.dt);
    const double dampF = md.damping[i] * vi;
    tau[(size_t)env * n + i] = s[L.rhs + i] + dampF + springF;
  }
  if (massMatrix != nullptr) {
    double* mm = massMatrix + (size_t)env * n * n;
    for (int t = lane; t < n * n; t += WAVE) {
      const int r = t / n, c = t - r * n;
      mm[t] = s[L.M + (r >= c ? tri(r, c) : tri(c, r))];
    }
  }
  if (bias != nullptr) {
    // a second pass of the accelerations with ddq = 0 and of the body forces
    // without the wrench (the composite inertias are dead: their area is the
    // accelerations' scratch, as in kinematics)
    ancestorAccelerations(md, s, L, lane, nullptr, s + L.IC);
    invDynBodyForces(md, s, L, lane, bi);
    for (int j = lane; j < n; j += WAVE)
      bias[(size_t)env * n + j] = dot6(s + L.Sw + 6 * j, s + L.F + 6 * md.dofBody[j]);
  }
}

// The vector-Jacobian product of tau = ID(q, v, a) with g = dL/dtau:
//   gradDdq   = M g
//   gradState = [(dID(q, v, a)/dq)^T g + K g,  (dC/dv)^T g + D g + dt K g]
//   gradWrench[b] = -(world twist of body b under the rate vector g), in the
//                   frame of the input (nullptr to skip); there is no dt
// With w := g and a* := a these are the step backward's adjoint vectors and
// per-dof columns (backwardItems: gq = -dt accQ - dt K w there): accQ =
// (dID/dq_k)^T w with the wrench terms of adjointVectors<kExt>, accV =
// (dC/dv_k)^T w, and M g = S_k . B, the subtree sum of beta = I W at the
// dof's body.  The kinematics are computed here (the step's backward reloads
// them from its snapshot); the per-dof columns are restated from
// backwardItems, which stays as it is.
// kInertia: one more output,
//   gradInertia[b][p] = W_b . phi_{b,p}    [B][nb][10], INERTIA_FULL order
// with W_b = sum of S_j g_j over the dofs of b and of its ancestors (the Wt of
// adjointVectors) and phi_{b,p} the derivative of the body's force with
// respect to its parameter p (inertia_grad.cuh): lane = body, all ten values
// of every device-model body, the massless frames of compound-joint chains
// included.  Damping, springs, the wrenches and dt do not enter.
template <bool kInertia = false>
__device__ __forceinline__ void invDynBackwardWorld(const ModelDev* __restrict__ mdp, const Layout& L,
                                                    const double* __restrict__ state,
                                                    const double* __restrict__ ddq,
                                                    const double* __restrict__ bodyInertia, int inertiaStride,
                                                    const double* __restrict__ bodyWrench, int wrenchStride,
                                                    int wrenchFrame, const double* __restrict__ gradTau,
                                                    double* __restrict__ gradState, double* __restrict__ gradDdq,
                                                    double* __restrict__ gradWrench,
                                                    double* __restrict__ gradInertia = nullptr) {
  extern __shared__ double s[];
  const ModelDev& md = *mdp;
  const int lane = threadIdx.x;
  const int n = md.n;
  const int env = blockIdx.x;
  {
    const double* st = state + (size_t)env * 2 * n;
    const double* a = ddq + (size_t)env * n;
    const double* g = gradTau + (size_t)env * n;
    for (int i = lane; i < n; i += WAVE) {
      s[L.q + i] = st[i];
      s[L.v + i] = st[n + i];
      s[L.x + i] = a[i];
      s[L.w + i] = g[i];
    }
    WSYNC();
  }
  // (L.IC, the scratch of the accelerations, is the adjoint area here)
  kinematics(md, s, L, lane, s + L.x);
  adjointVectors<true, true>(md, s, L, lane, bodyInertia + (size_t)env * inertiaStride,
                             bodyWrench + (size_t)env * wrenchStride, wrenchFrame);
  if (gradWrench != nullptr && lane < md.nb) {
    const int b = lane;
    double Wd[6], gw[6];
    for (int i = 0; i < 6; i++) Wd[i] = -s[L.Wt + 6 * b + i];
    twistInWrenchFrame(Wd, wrenchFrame, s + L.Tw + 12 * b, gw);
    for (int i = 0; i < 6; i++) gradWrench[((size_t)env * md.nb + b) * 6 + i] = gw[i];
  }
  if constexpr (kInertia) {
    if (lane < md.nb) {
      const int b = lane;
      const double* bi = bodyInertia + (size_t)env * inertiaStride + 10 * b;
      const double ag[6] = {0, 0, 0, md.g[0], md.g[1], md.g[2]};
      double u[6];
      for (int i = 0; i < 6; i++) u[i] = s[L.A + 6 * b + i] - ag[i];
      double* gi = gradInertia + ((size_t)env * md.nb + b) * 10;
#pragma unroll
      for (int p = 0; p < 10; p++)
        gi[p] = inertiaPhiDot(s + L.Tw + 12 * b, bi[0], bi + 1, s + L.V + 6 * b, u, s + L.Wt + 6 * b, p);
    }
  }
  const int k = lane;
  if (k < n) {
    const int b = md.dofBody[k];
    const int lam = md.parent[b];
    const double ag[6] = {0, 0, 0, md.g[0], md.g[1], md.g[2]};
    double Vl[6], ul[6];
    for (int i = 0; i < 6; i++) {
      Vl[i] = lam >= 0 ? s[L.V + 6 * lam + i] : 0.0;
      ul[i] = (lam >= 0 ? s[L.A + 6 * lam + i] : 0.0) - ag[i];
    }
    // position generator Z (world twist of the subtree per unit q_k)
    double Z[6] = {0, 0, 0, 0, 0, 0};
    const double* Sk = s + L.Sw + 6 * k;
    if (md.jtype[b] == NIMBLE_JOINT_FREE || md.jtype[b] == NIMBLE_JOINT_BALL) {
      const int o = md.dof0[b];
      const int c = k - o;
      double xi[6] = {0, 0, 0, 0, 0, 0};
      const double* th = s + L.q + o;
      if (c < 3) {
        rightJacobianCol(th, c, xi);
      } else {
        double Rm[9];
        expMapRot(th, Rm);
        for (int r = 0; r < 3; r++) xi[3 + r] = Rm[(c - 3) * 3 + r];  // R^T e_c
      }
      double TwC[12];
      tmul(s + L.Tw + 12 * b, md.Tcj[b], TwC);
      adT(TwC, xi, Z);
    } else {
      for (int i = 0; i < 6; i++) Z[i] = Sk[i];
    }
    // adjoint contraction at body b (subtree sums, see adjointVectors)
    const double* a = s + L.adj + 42 * b;
    double t[6], r[6], acc6[6];
    crf(Vl, a + 6, t);  // V_l x* B
    for (int i = 0; i < 6; i++) r[i] = a[12 + i] + t[i] + a[24 + i] - a[30 + i];
    crf(Vl, r, t);
    crf(ul, a + 6, r);  // u_l x* B
    for (int i = 0; i < 6; i++) acc6[i] = -a[i] - r[i] + t[i] + a[18 + i] + a[36 + i];
    const double accQ = dot6(Z, acc6);
    double vs[6];
    for (int i = 0; i < 6; i++) vs[i] = Vl[i] + s[L.V + 6 * b + i];
    crf(vs, a + 6, t);
    for (int i = 0; i < 6; i++) acc6[i] = -t[i] - a[12 + i] - a[24 + i] + a[30 + i];
    const double accV = dot6(Sk, acc6);
    const double wk = s[L.w + k];
    double* gs = gradState + (size_t)env * 2 * n;
    gs[k] = accQ + md.spring[k] * wk;
    gs[n + k] = accV + md.damping[k] * wk + md.dt * md.spring[k] * wk;
    gradDdq[(size_t)env * n + k] = dot6(Sk, a + 6);
  }
}

// jacobian [B][n][nb][10]: d tau_j / d theta_{b,p} = S_j . phi_{b,p} where dof
// j belongs to body b or to one of its ancestors, exactly 0.0 elsewhere --
// Skeleton::getJacobianOfID(ddq, wrt) = getJacobianOfM(ddq, wrt) +
// getJacobianOfC(wrt) (Skeleton.cpp:1884, :1832, :1779) for wrt = GROUP_MASSES,
// GROUP_COMS and GROUP_INERTIAS at once, over all of the world's bodies.  Only
// the kinematics with ddq = a run (Tw, Sw, V, A on the forward's lean layout;
// no composites, no M).  One lane per element, in the order of the output:
// neighbouring lanes store neighbouring addresses, every element is written
// (the caller's memory may be uninitialised), and a lane holds one value of
// one parameter at a time, never a body's ten 6-vectors phi.
__device__ __forceinline__ void invDynInertiaJacobianWorld(const ModelDev* __restrict__ mdp, const Layout& L,
                                                           const double* __restrict__ state,
                                                           const double* __restrict__ ddq,
                                                           const double* __restrict__ bodyInertia,
                                                           int inertiaStride, double* __restrict__ jacobian) {
  extern __shared__ double s[];
  const ModelDev& md = *mdp;
  const int lane = threadIdx.x;
  const int n = md.n;
  const int env = blockIdx.x;
  {
    const double* st = state + (size_t)env * 2 * n;
    const double* a = ddq + (size_t)env * n;
    for (int i = lane; i < n; i += WAVE) {
      s[L.q + i] = st[i];
      s[L.v + i] = st[n + i];
      s[L.x + i] = a[i];
    }
    WSYNC();
  }
  kinematics(md, s, L, lane, s + L.x);
  const double* bi = bodyInertia + (size_t)env * inertiaStride;
  const double ag[6] = {0, 0, 0, md.g[0], md.g[1], md.g[2]};
  const int row = 10 * md.nb, total = n * row;
  double* J = jacobian + (size_t)env * total;
  for (int t = lane; t < total; t += WAVE) {
    const int j = t / row, r = t - j * row;
    const int b = r / 10, p = r - 10 * b;
    double val = 0.0;
    if ((md.anc[b] >> md.dofBody[j]) & 1ull) {
      double u[6];
      for (int i = 0; i < 6; i++) u[i] = s[L.A + 6 * b + i] - ag[i];
      val = inertiaPhiDot(s + L.Tw + 12 * b, bi[10 * b], bi + 10 * b + 1, s + L.V + 6 * b, u, s + L.Sw + 6 * j, p);
    }
    J[t] = val;
  }
}

// (the kernels: the workgroup's dynamic LDS is declared in the functions
// above, as in the step's kernels)
extern "C" __global__ void __launch_bounds__(WAVE)
nimble_inverse_dynamics_kernel(const ModelDev* __restrict__ mdp, Layout L, const double* __restrict__ state,
                               const double* __restrict__ ddq, const double* __restrict__ bodyInertia,
                               int inertiaStride, const double* __restrict__ bodyWrench, int wrenchStride,
                               int wrenchFrame, double* __restrict__ tau, double* __restrict__ massMatrix,
                               double* __restrict__ bias) {
  invDynWorld(mdp, L, state, ddq, bodyInertia, inertiaStride, bodyWrench, wrenchStride, wrenchFrame, tau, massMatrix,
              bias);
}

extern "C" __global__ void __launch_bounds__(WAVE)
nimble_inverse_dynamics_backward_kernel(const ModelDev* __restrict__ mdp, Layout L, const double* __restrict__ state,
                                        const double* __restrict__ ddq, const double* __restrict__ bodyInertia,
                                        int inertiaStride, const double* __restrict__ bodyWrench, int wrenchStride,
                                        int wrenchFrame, const double* __restrict__ gradTau,
                                        double* __restrict__ gradState, double* __restrict__ gradDdq,
                                        double* __restrict__ gradWrench) {
  invDynBackwardWorld<false>(mdp, L, state, ddq, bodyInertia, inertiaStride, bodyWrench, wrenchStride, wrenchFrame,
                             gradTau, gradState, gradDdq, gradWrench);
}

extern "C" __global__ void __launch_bounds__(WAVE)
nimble_inverse_dynamics_backward_inertia_kernel(const ModelDev* __restrict__ mdp, Layout L,
                                                const double* __restrict__ state, const double* __restrict__ ddq,
                                                const double* __restrict__ bodyInertia, int inertiaStride,
                                                const double* __restrict__ bodyWrench, int wrenchStride,
                                                int wrenchFrame, const double* __restrict__ gradTau,
                                                double* __restrict__ gradState, double* __restrict__ gradDdq,
                                                double* __restrict__ gradWrench, double* __restrict__ gradInertia) {
  invDynBackwardWorld<true>(mdp, L, state, ddq, bodyInertia, inertiaStride, bodyWrench, wrenchStride, wrenchFrame,
                            gradTau, gradState, gradDdq, gradWrench, gradInertia);
}

extern "C" __global__ void __launch_bounds__(WAVE)
nimble_inverse_dynamics_inertia_jacobian_kernel(const ModelDev* __restrict__ mdp, Layout L,
                                                const double* __restrict__ state, const double* __restrict__ ddq,
                                                const double* __restrict__ bodyInertia, int inertiaStride,
                                                double* __restrict__ jacobian) {
  invDynInertiaJacobianWorld(mdp, L, state, ddq, bodyInertia, inertiaStride, jacobian);
}
