// The contact inverse-dynamics kernel (contact_inverse_dynamics.cuh, through
// timestep.hip's host build, which takes every kernel set) and its C-ABI entry
// point (capi.cpp) compiled for the host against the execution-model
// emulation in hip/hip_runtime.h (test infrastructure only): reads a world
// description and inputs written by tests/test_contact_inverse_dynamics_emu.py
// and runs nimble_contact_inverse_dynamics through the C-ABI exactly as on the
// GPU.  For the test's numpy reference it also prints, from the existing
// entry points, the plain inverse dynamics of the same inputs and the bodies'
// Jacobians (nimble_inverse_dynamics_backward with unit grad_tau: grad_wrench
// in body frame is minus the Jacobian's column).  Built with
// AddressSanitizer: any out-of-bounds access of the kernel on these inputs
// aborts the run with its location.
//
// input (whitespace-separated): the world description of step_emu.cpp, then
//   B  state[B 2n]  ddq[B n]  wrench_frame  body_wrench[B nb 6]
//   k  bodies[k]  has_guesses  guesses[B k 6] (when has_guesses)
// output lines: "tau" [B n], "F" [B k 6], "full" [B n], "gw" [B n nb 6]
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
  const int frame = readArr<int>(1)[0];
  auto wrench = readArr<double>((size_t)B * nb * 6);
  const int k = readArr<int>(1)[0];
  auto bodies = readArr<int32_t>(k);
  const int hasGuess = readArr<int>(1)[0];
  std::vector<double> guess;
  if (hasGuess) guess = readArr<double>((size_t)B * k * 6);
  // exact-size heap buffers: a write past any of them is an ASan report
  std::vector<double> tau((size_t)B * n), F((size_t)B * k * 6), full((size_t)B * n);
  if (nimble_contact_inverse_dynamics(w, B, state.data(), ddq.data(), nullptr, wrench.data(), frame, k, bodies.data(),
                                      hasGuess ? guess.data() : nullptr, tau.data(), F.data(), nullptr) != NIMBLE_OK) {
    std::fprintf(stderr, "contact inverse dynamics: %s\n", nimble_last_error());
    return 4;
  }
  print("tau", tau);
  print("F", F);
  if (nimble_inverse_dynamics(w, B, state.data(), ddq.data(), nullptr, wrench.data(), frame, full.data(), nullptr,
                              nullptr, nullptr) != NIMBLE_OK) {
    std::fprintf(stderr, "inverse dynamics: %s\n", nimble_last_error());
    return 5;
  }
  print("full", full);
  // the Jacobians: one backward item per (world, dof) with grad_tau = e_dof
  // and a zero body-frame wrench
  const size_t items = (size_t)B * n;
  std::vector<double> st2(items * 2 * n), a2(items * n), g2(items * n, 0.0), z(items * nb * 6, 0.0);
  for (int b = 0; b < B; b++)
    for (int j = 0; j < n; j++) {
      const size_t it = (size_t)b * n + j;
      for (int i = 0; i < 2 * n; i++) st2[it * 2 * n + i] = state[(size_t)b * 2 * n + i];
      for (int i = 0; i < n; i++) a2[it * n + i] = ddq[(size_t)b * n + i];
      g2[it * n + j] = 1.0;
    }
  std::vector<double> gs(items * 2 * n), ga(items * n), gw(items * nb * 6);
  if (nimble_inverse_dynamics_backward(w, (int)items, st2.data(), a2.data(), nullptr, z.data(), NIMBLE_WRENCH_BODY,
                                       g2.data(), gs.data(), ga.data(), gw.data(), nullptr) != NIMBLE_OK) {
    std::fprintf(stderr, "inverse dynamics backward: %s\n", nimble_last_error());
    return 6;
  }
  print("gw", gw);
  nimble_world_destroy(w);
  return 0;
}
