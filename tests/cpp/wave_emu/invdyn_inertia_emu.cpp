// The two inverse-dynamics kernels for the inertial parameters
// (inverse_dynamics.cuh: nimble_inverse_dynamics_backward_inertia_kernel and
// nimble_inverse_dynamics_inertia_jacobian_kernel, through timestep.hip's host
// build, which takes every kernel set) and their C-ABI entry points (capi.cpp)
// compiled for the host against the execution-model emulation in
// hip/hip_runtime.h (test infrastructure only): reads a world description and
// inputs written by tests/test_inverse_dynamics_inertia_emu.py, runs
// nimble_invdyn_inertia_jacobian and nimble_invdyn_backward_inertia through
// the C-ABI exactly as on the GPU, with per-world parameter rows, and prints
// the results.  Built with AddressSanitizer: any out-of-bounds access of the
// kernels on these inputs aborts the run with its location.
//
// input (whitespace-separated): the world description of step_emu.cpp, then
//   B  state[B 2n]  ddq[B n]  grad_tau[B n]  body_inertia[B nb 10]
// output lines: "jac" [B n nb 10], "gi" [B nb 10], "gs" [B 2n], "ga" [B n]
// (nimble_invdyn_backward_inertia), "gs0" [B 2n], "ga0" [B n]
// (nimble_inverse_dynamics_backward on the same inputs)
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

double s[160 * 1024 / 8];  // the workgroup's LDS (dynamic shared memory)

#include "../../../nimblephysics_amd/csrc/timestep.hip"
#include "../../../nimblephysics_amd/csrc/capi.cpp"

template <class T>
static std::vector<T> readArr(size_t n) {
  std::vector<T> v(n);
  for (auto& x : v) {
    std::string t;
    if (!(std::cin >> t)) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    if constexpr (std::is_same<T, double>::value) x = std::strtod(t.c_str(), nullptr);
    else x = (T)std::strtol(t.c_str(), nullptr, 10);
  }
  return v;
}

static void print(const char* key, const std::vector<double>& v) {
  std::printf("%s", key);
  for (double x : v) std::printf(" %.17g", x);
  std::printf("\n");
}

int main() {
  auto hi = readArr<int>(7);
  auto hd = readArr<double>(6);
  const int nb = hi[0], n = hi[1], ns = hi[2], nmv = hi[3];
  auto parent = readArr<int32_t>(nb), skel = readArr<int32_t>(nb), jt = readArr<int32_t>(nb);
  auto dof0 = readArr<int32_t>(nb), mobile = readArr<int32_t>(nb);
  auto Tp = readArr<double>(12 * nb), Tc = readArr<double>(12 * nb), axis = readArr<double>(3 * nb);
  auto mass = readArr<double>(nb), com = readArr<double>(3 * nb), moment = readArr<double>(6 * nb);
  auto fric = readArr<double>(nb), rest = readArr<double>(nb);
  std::vector<std::vector<double>> dofs;
  for (int k = 0; k < 9; k++) dofs.push_back(readArr<double>(n));
  auto sb = readArr<int32_t>(ns), st = readArr<int32_t>(ns);
  auto ssz = readArr<double>(3 * ns), sT = readArr<double>(12 * ns);
  auto mf = readArr<int32_t>(ns), mc = readArr<int32_t>(ns);
  auto mv = readArr<double>(3 * (size_t)nmv);
  std::vector<int32_t> cand;
  if (hi[6]) cand = readArr<int32_t>(nmv);
  nimble_world_desc d{};
  d.num_bodies = nb; d.num_dofs = n; d.num_shapes = ns;
  d.dt = hd[0]; d.gravity[0] = hd[1]; d.gravity[1] = hd[2]; d.gravity[2] = hd[3];
  d.contact_clipping_depth = hd[4]; d.fallback_cfm = hd[5];
  d.penetration_correction = hi[4]; d.parallel_pos_vel = hi[5];
  d.parent = parent.data(); d.skeleton = skel.data(); d.joint_type = jt.data(); d.dof_offset = dof0.data();
  d.skeleton_mobile = mobile.data(); d.T_parent_joint = Tp.data(); d.T_child_joint = Tc.data();
  d.axis = axis.data(); d.mass = mass.data(); d.com = com.data(); d.moment = moment.data();
  d.friction = fric.data(); d.restitution = rest.data();
  d.damping = dofs[0].data(); d.spring = dofs[1].data(); d.rest_position = dofs[2].data();
  d.pos_lower = dofs[3].data(); d.pos_upper = dofs[4].data(); d.vel_lower = dofs[5].data();
  d.vel_upper = dofs[6].data(); d.force_lower = dofs[7].data(); d.force_upper = dofs[8].data();
  d.shape_body = sb.data(); d.shape_type = st.data(); d.shape_size = ssz.data(); d.shape_T = sT.data();
  d.num_mesh_vertices = nmv; d.mesh_vertices = nmv ? mv.data() : nullptr;
  d.shape_mesh_first = mf.data(); d.shape_mesh_count = mc.data();
  d.mesh_vertex_candidate = hi[6] ? cand.data() : nullptr;
  nimble_world_t w = nullptr;
  if (nimble_world_create(&d, &w) != NIMBLE_OK) {
    std::fprintf(stderr, "create: %s\n", nimble_last_error());
    return 3;
  }
  const int B = readArr<int>(1)[0];
  auto state = readArr<double>((size_t)B * 2 * n), ddq = readArr<double>((size_t)B * n);
  auto grad = readArr<double>((size_t)B * n);
  auto params = readArr<double>((size_t)B * nb * 10);
  // exact-size heap buffers: a write past any of them is an ASan report;
  // the outputs start as NaN: every element has to be written
  const double nan = std::nan("");
  std::vector<double> jac((size_t)B * n * nb * 10, nan), gi((size_t)B * nb * 10, nan);
  std::vector<double> gs((size_t)B * 2 * n, nan), ga((size_t)B * n, nan), gs0(gs), ga0(ga);
  if (nimble_invdyn_inertia_jacobian(w, B, state.data(), ddq.data(), params.data(), jac.data(), nullptr) !=
          NIMBLE_OK ||
      nimble_invdyn_backward_inertia(w, B, state.data(), ddq.data(), params.data(), nullptr, NIMBLE_WRENCH_WORLD,
                                     grad.data(), gs.data(), ga.data(), nullptr, gi.data(), nullptr) != NIMBLE_OK ||
      nimble_inverse_dynamics_backward(w, B, state.data(), ddq.data(), params.data(), nullptr, NIMBLE_WRENCH_WORLD,
                                       grad.data(), gs0.data(), ga0.data(), nullptr, nullptr) != NIMBLE_OK) {
    std::fprintf(stderr, "inverse dynamics, inertial parameters: %s\n", nimble_last_error());
    return 4;
  }
  // the required outputs
  if (nimble_invdyn_inertia_jacobian(w, B, state.data(), ddq.data(), nullptr, nullptr, nullptr) !=
          NIMBLE_ERR_INVALID ||
      nimble_invdyn_backward_inertia(w, B, state.data(), ddq.data(), nullptr, nullptr, NIMBLE_WRENCH_WORLD,
                                     grad.data(), gs.data(), ga.data(), nullptr, nullptr, nullptr) !=
          NIMBLE_ERR_INVALID) {
    std::fprintf(stderr, "a NULL jacobian / grad_inertia was accepted\n");
    return 5;
  }
  print("jac", jac);
  print("gi", gi);
  print("gs", gs);
  print("ga", ga);
  print("gs0", gs0);
  print("ga0", ga0);
  nimble_world_destroy(w);
  return 0;
}
