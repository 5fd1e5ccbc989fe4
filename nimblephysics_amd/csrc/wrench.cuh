// External body wrenches (body_wrench [batch][num_bodies][6] of the `_ext`
// entry points, include/nimble_amd.h): the reference's BodyNode::mFext
// (dart/dynamics/BodyNode.cpp:1532-1612), which enters the bias force as
// `- mFext` (:2079), and the worldWrench of DifferentiableExternalForce
// (dart/neural/DifferentiableExternalForce.cpp:58).  Six doubles per body,
// [torque xyz, force xyz] -- the spatial order of Sw, V and F in the kernels.
// The kernels work in world axes about the world origin; the two helpers take
// a body-frame wrench there and a world twist back, with the body's world
// transform Tw (3x4 row-major [R|p], in LDS).  Every read is a load at the
// point of use: nothing is staged in LDS by this file.
#pragma once

#include "model.h"
#include "spatial.cuh"

// World-frame wrench of body b from its six values `f`.
// NIMBLE_WRENCH_WORLD: as given.  NIMBLE_WRENCH_BODY: dAdInvT(Tw, f) =
// [R t + p x (R f_lin); R f_lin].  `frame` is wave-uniform.
__device__ __forceinline__ void worldWrench(const double* f, int frame, const double* Tw, double* o) {
  if (frame == NIMBLE_WRENCH_WORLD) {
    for (int i = 0; i < 6; i++) o[i] = f[i];
    return;
  }
  double rt[3], rf[3], px[3];
  for (int r = 0; r < 3; r++) {
    rt[r] = Tw[r * 4] * f[0] + Tw[r * 4 + 1] * f[1] + Tw[r * 4 + 2] * f[2];
    rf[r] = Tw[r * 4] * f[3] + Tw[r * 4 + 1] * f[4] + Tw[r * 4 + 2] * f[5];
  }
  const double p[3] = {Tw[3], Tw[7], Tw[11]};
  cross3(p, rf, px);
  for (int r = 0; r < 3; r++) {
    o[r] = rt[r] + px[r];
    o[3 + r] = rf[r];
  }
}

// The world twist V = [w; v] (about the world origin) in the frame of the
// wrench input: as it is, or Ad_{Tw^-1} V = [R^T w; R^T (v + w x p)], the
// transpose of the map above (wrench . twist is the same in both frames).
__device__ __forceinline__ void twistInWrenchFrame(const double* V, int frame, const double* Tw, double* o) {
  if (frame == NIMBLE_WRENCH_WORLD) {
    for (int i = 0; i < 6; i++) o[i] = V[i];
    return;
  }
  const double p[3] = {Tw[3], Tw[7], Tw[11]};
  double wxp[3], u[3];
  cross3(V, p, wxp);
  for (int i = 0; i < 3; i++) u[i] = V[3 + i] + wxp[i];
  for (int i = 0; i < 3; i++) {
    o[i] = Tw[i] * V[0] + Tw[4 + i] * V[1] + Tw[8 + i] * V[2];
    o[3 + i] = Tw[i] * u[0] + Tw[4 + i] * u[1] + Tw[8 + i] * u[2];
  }
}
