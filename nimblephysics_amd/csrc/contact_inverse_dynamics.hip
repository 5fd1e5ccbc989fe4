// The contact inverse-dynamics kernel (include/nimble_amd.h
// nimble_contact_inverse_dynamics; contact_inverse_dynamics.cuh):
// nimble_contact_inverse_dynamics_kernel.  It shares timestep.hip's
// kinematics, composites and mass matrix and chol_wave.cuh's factorisation,
// and is compiled here, into a code object of its own that holds none of the
// other kernels, so that those stay what they are without it (see the note at
// the top of timestep.hip).
#define NIMBLE_CONTACT_ID_KERNELS
#include "timestep.hip"
