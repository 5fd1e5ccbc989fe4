// Derivatives of a body's force with respect to its inertial parameters, for
// the inverse-dynamics kernels (inverse_dynamics.cuh): the entries of the
// reference's Skeleton::getJacobianOfID(x, wrt) = getJacobianOfM(x, wrt) +
// getJacobianOfC(wrt) (dart/dynamics/Skeleton.cpp:1884, :1832, :1779) with wrt
// = GROUP_MASSES, GROUP_COMS, GROUP_INERTIAS, in world coordinates.
//
// Body b has the parameters theta (INERTIA_FULL order, WithRespectToMass.cpp:35:
// mass, local COM x y z, moment about the COM Ixx Iyy Izz Ixy Ixz Iyz), the
// world-frame spatial inertia G, the twist V and u = A - a_g (its acceleration
// less gravity).  Its force f = G u + V x* (G V) has
//   phi_p = df/dtheta_p = (dG/dtheta_p) u + V x* ((dG/dtheta_p) V)
// and, for any twist x, because x . (V x* h) = -(V x x) . h,
//   x . phi_p = x^T (dG/dtheta_p) u - (V x x)^T (dG/dtheta_p) V:
// two values of the symmetric bilinear form x^T (dG/dtheta_p) y.  With twists
// x = [w_x; v_x], the COM c in the world, its velocity u_x = v_x - c x w_x and
// the body-frame angular part wb_x = R^T w_x,
//   x^T G y = wb_x^T I wb_y + m u_x . u_y
// so
//   d/dm     u_x . u_y
//   d/dc_k   m ((w_x x r_k) . u_y + u_x . (w_y x r_k)),  r_k = R e_k
//   d/dI_ij  wb_x,i wb_y,j  (+ wb_x,j wb_y,i off the diagonal)
// -- the closed forms of the step's gradient in the inertial parameters
// (timestep.hip, nimble_backward_inertia), restated here without its factor
// -dt and its contact pairs; that code stays as it is.
#pragma once

// b[i] for a run-time i without indexing a register array
__device__ __forceinline__ double inertiaGradPick(const double* b, int i) {
  return i == 0 ? b[0] : (i == 1 ? b[1] : b[2]);
}

// x^T (dG/dtheta_p) y.  Tw: the body's world transform (row-major 3x4, read
// with a run-time column index: keep it in memory), cw: its COM in the world.
__device__ __forceinline__ double inertiaPairTerm(const double* Tw, double m, const double* cw, const double* x,
                                                  const double* y, int p) {
  if (p < 4) {
    double cx[3], ux[3], uy[3];
    cross3(cw, x, cx);
    for (int i = 0; i < 3; i++) ux[i] = x[3 + i] - cx[i];
    cross3(cw, y, cx);
    for (int i = 0; i < 3; i++) uy[i] = y[3 + i] - cx[i];
    if (p == 0) return dot3(ux, uy);
    const int k = p - 1;
    const double rk[3] = {Tw[k], Tw[4 + k], Tw[8 + k]};
    double a[3], c[3];
    cross3(x, rk, a);  // w_x x r_k
    cross3(y, rk, c);  // w_y x r_k
    return m * (dot3(a, uy) + dot3(ux, c));
  }
  double bx[3], by[3];  // R^T w_x, R^T w_y
  for (int i = 0; i < 3; i++) {
    bx[i] = Tw[i] * x[0] + Tw[4 + i] * x[1] + Tw[8 + i] * x[2];
    by[i] = Tw[i] * y[0] + Tw[4 + i] * y[1] + Tw[8 + i] * y[2];
  }
  if (p < 7) return inertiaGradPick(bx, p - 4) * inertiaGradPick(by, p - 4);
  // Ixy, Ixz, Iyz: (i, j) = (0, 1), (0, 2), (1, 2)
  const int i = p == 9 ? 1 : 0, j = p == 7 ? 1 : 2;
  return inertiaGradPick(bx, i) * inertiaGradPick(by, j) + inertiaGradPick(bx, j) * inertiaGradPick(by, i);
}

// x . phi_p of one body: Tw its world transform, m and cb its mass and local
// COM, V its twist, u = A - a_g, p = 0 .. 9.  In a loop over a compile-time p
// the shared subexpressions are formed once.
__device__ __forceinline__ double inertiaPhiDot(const double* Tw, double m, const double* cb, const double* V,
                                                const double* u, const double* x, int p) {
  double cw[3], Vx[6];
  for (int r = 0; r < 3; r++) cw[r] = Tw[r * 4] * cb[0] + Tw[r * 4 + 1] * cb[1] + Tw[r * 4 + 2] * cb[2] + Tw[r * 4 + 3];
  crm(V, x, Vx);
  return inertiaPairTerm(Tw, m, cw, x, u, p) - inertiaPairTerm(Tw, m, cw, Vx, V, p);
}
