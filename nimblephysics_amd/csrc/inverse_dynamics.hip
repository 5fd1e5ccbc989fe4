// The inverse-dynamics kernels (include/nimble_amd.h nimble_inverse_dynamics,
// nimble_inverse_dynamics_backward, nimble_invdyn_backward_inertia,
// nimble_invdyn_inertia_jacobian; inverse_dynamics.cuh):
// nimble_inverse_dynamics_kernel, nimble_inverse_dynamics_backward_kernel,
// nimble_inverse_dynamics_backward_inertia_kernel and
// nimble_inverse_dynamics_inertia_jacobian_kernel.
// They share timestep.hip's kinematics, composites, mass matrix and adjoint
// vectors, and are compiled here, into a code object of their own that holds
// none of the step's kernels, so that those stay what they are without them
// (see the note at the top of timestep.hip).
#define NIMBLE_INVERSE_DYNAMICS_KERNELS
#include "timestep.hip"
