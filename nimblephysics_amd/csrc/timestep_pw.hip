// The kernel instances that read every body's inertial parameters from the
// per-world array body_inertia [batch][num_bodies][10] (include/nimble_amd.h,
// the _pw entry points): nimble_forward_pw_kernel,
// nimble_forward_mesh_pw_kernel, nimble_backward_pw_kernel and
// nimble_backward_wide_pw_kernel.  Their source is timestep.hip's, with the
// template parameter kPW set; they are compiled here, into a code object of
// their own, so that the shared-model kernels stay what they are without
// them (see the note at the top of timestep.hip).
#define NIMBLE_PER_WORLD_KERNELS
#include "timestep.hip"
