// The kernel instances that take external body wrenches, body_wrench
// [batch][num_bodies][6] (include/nimble_amd.h, the _ext entry points;
// wrench.cuh): nimble_forward_ext_kernel, nimble_forward_mesh_ext_kernel,
// nimble_backward_ext_kernel and nimble_backward_wide_ext_kernel.  Their
// source is timestep.hip's, with the template parameters kExt and kPW set;
// they are compiled here, into a code object of their own, so that the other
// kernels stay what they are without them (see the note at the top of
// timestep.hip).
#define NIMBLE_EXT_WRENCH_KERNELS
#include "timestep.hip"
