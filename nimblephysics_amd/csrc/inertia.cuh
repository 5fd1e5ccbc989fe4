// Where a kernel reads a body's inertial parameters from.
//
// BodyInertia<false>: the shared device model (ModelDev::mass / com / Ic), the
// reads the kernels have always made.  BodyInertia<true>: the world's own row
// of the per-world array `body_inertia` [batch][num_bodies][10]
// (include/nimble_amd.h), ten doubles per body in WithRespectToMass's
// INERTIA_FULL order (dart/neural/WithRespectToMass.cpp:35-181): mass, local
// COM x y z, moment about the COM Ixx Iyy Izz Ixy Ixz Iyz.  Ic(i) is element
// i of the symmetric 3x3 in row-major order, filled from the six moments by
// placement only, as nimble_world_create fills ModelDev::Ic.  Every accessor
// is a load at the point of use: nothing is staged in LDS or kept in
// registers by this type, and the arithmetic of the reading site is the same
// for both sources.
#pragma once

#include "model.h"

template <bool kPW>
struct BodyInertia;

template <>
struct BodyInertia<false> {
  const ModelDev& md;
  const int b;
  __device__ __forceinline__ BodyInertia(const ModelDev& m, const double*, int body) : md(m), b(body) {}
  __device__ __forceinline__ double mass() const { return md.mass[b]; }
  __device__ __forceinline__ double com(int i) const { return md.com[b][i]; }
  __device__ __forceinline__ double Ic(int i) const { return md.Ic[b][i]; }
};

template <>
struct BodyInertia<true> {
  const double* p;  // the body's ten values
  __device__ __forceinline__ BodyInertia(const ModelDev&, const double* world, int body) : p(world + 10 * body) {}
  __device__ __forceinline__ double mass() const { return p[0]; }
  __device__ __forceinline__ double com(int i) const { return p[1 + i]; }
  __device__ __forceinline__ double Ic(int i) const {
    // [Ixx Ixy Ixz; Ixy Iyy Iyz; Ixz Iyz Izz] from (Ixx Iyy Izz Ixy Ixz Iyz)
    const int at[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
    return p[4 + at[i]];
  }
};
