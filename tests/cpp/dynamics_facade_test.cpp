// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::inverseDynamics / forwardDynamics (all envs in one call, computed on
// the device) against the C-ABI they wrap - bit for bit, on host buffers - with the state rows STAGED through per-env views, which the batched members
// have to upload first: a second world that was given the same rows through rsb_set_state answers with the same bits.  The round trip
// inverseDynamics(forwardDynamics(tau)) returns tau within 2e-5 (1 + the env's largest |tau|, |udot| row scale).
// Exit code 0 = all checks passed, 1 = a check failed or no device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/World.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
unsigned g_seed = 4242u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * 4); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: dynamics_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 21;      // two workgroups of 19 ANYmal envs, the second with a tail
    raisim::BatchedWorld batch(urdf, N), twin(urdf, N);
    const int nq = batch.gcDim(), nv = batch.dof(), nb = batch.blob().nb;
    std::vector<std::unique_ptr<raisim::World>> views;
    std::vector<float> gc((size_t)N * nq), gv((size_t)N * nv);
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      raisim::ArticulatedSystem* robot = views.back()->addArticulatedSystem(urdf);
      raisim::VecDyn g(nq), v(nv);
      double q4[4], n2 = 0;
      for (double& x : q4) { x = 2 * uni() - 1; n2 += x * x; }
      g[0] = 4 * uni() - 2 + (e % 4 == 0 ? 50.0 : 0.0); g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 2 * uni() - 1;
      for (int k = 0; k < nv; ++k) v[k] = 4 * uni() - 2;
      robot->setState(g, v);        // staged through the view: the batched calls below must see it
      for (int k = 0; k < nq; ++k) gc[(size_t)e * nq + k] = (float)g[k];
      for (int k = 0; k < nv; ++k) gv[(size_t)e * nv + k] = (float)v[k];
    }
    RSB_CHECK(rsb_set_state(twin.handle(), gc.data(), gv.data(), nullptr, RSB_HOST));
    const std::vector<rsb_frame> frames = {{nb - 1, {0.05f, -0.02f, 0.1f}}, {nb - 1, {-0.1f, 0.03f, 0.f}}, {nb / 2, {0.f, 0.04f, -0.06f}}};
    const int F = (int)frames.size();
    std::vector<float> udot((size_t)N * nv), tau((size_t)N * nv), force((size_t)N * F * 3), torque((size_t)N * F * 3);
    for (float& x : udot) x = (float)(4 * uni() - 2);
    for (float& x : tau) x = (float)(4 * uni() - 2);
    for (float& x : force) x = (float)(4 * uni() - 2);
    for (float& x : torque) x = (float)(4 * uni() - 2);
    const size_t w3 = (size_t)N * nb * 3;
    std::vector<float> t1((size_t)N * nv), f1(w3), n1(w3), a1((size_t)N * nv), t2(t1.size()), f2(w3), n2(w3), a2(a1.size());
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.inverseDynamics(udot.data(), frames, force.data(), torque.data(), false, t1.data(), f1.data(), n1.data());
    RSB_CHECK(rsb_inverse_dynamics(twin.handle(), udot.data(), frames.data(), F, force.data(), torque.data(), 0, t2.data(), f2.data(), n2.data(), RSB_HOST));
    CHECK(same(t1, t2) && same(f1, f2) && same(n1, n2));
    batch.forwardDynamics(tau.data(), frames, force.data(), torque.data(), false, a1.data());
    RSB_CHECK(rsb_forward_dynamics(twin.handle(), tau.data(), frames.data(), F, force.data(), torque.data(), 0, a2.data(), RSB_HOST));
    CHECK(same(a1, a2));
    // ... and the members are the C-ABI's calls on the facade's own world: the same bits again
    RSB_CHECK(rsb_inverse_dynamics(batch.handle(), udot.data(), frames.data(), F, force.data(), torque.data(), 0, t2.data(), f2.data(), n2.data(), RSB_HOST));
    RSB_CHECK(rsb_forward_dynamics(batch.handle(), tau.data(), frames.data(), F, force.data(), torque.data(), 0, a2.data(), RSB_HOST));
    CHECK(same(t1, t2) && same(f1, f2) && same(n1, n2) && same(a1, a2));
    // null outputs are skipped, no loads and no udot are valid calls
    std::vector<float> only(w3, 7.f), h1((size_t)N * nv), h2(h1.size());
    batch.inverseDynamics(udot.data(), frames, force.data(), torque.data(), false, nullptr, nullptr, only.data());
    CHECK(same(only, n1));
    batch.inverseDynamics(nullptr, {}, nullptr, nullptr, true, h1.data(), nullptr, nullptr);      // (no contacts yet: nothing has stepped)
    RSB_CHECK(rsb_inverse_dynamics(batch.handle(), nullptr, nullptr, 0, nullptr, nullptr, 0, h2.data(), nullptr, nullptr, RSB_HOST));
    CHECK(same(h1, h2));
    // round trip: the force that produces the acceleration the force produced
    batch.inverseDynamics(a1.data(), frames, force.data(), torque.data(), false, t2.data(), nullptr, nullptr);
    double worst = 0;
    for (int e = 0; e < N; ++e) {
      double scale = 0, err = 0;
      for (int k = 0; k < nv; ++k) {
        scale = std::max(scale, std::max((double)std::fabs(t1[(size_t)e * nv + k]), std::max((double)std::fabs(tau[(size_t)e * nv + k]), (double)std::fabs(a1[(size_t)e * nv + k]))));
        err = std::max(err, (double)std::fabs(t2[(size_t)e * nv + k] - tau[(size_t)e * nv + k]));
      }
      worst = std::max(worst, err / (2e-5 * (1 + scale)));
      if (!(err <= 2e-5 * (1 + scale))) { std::printf("env %d: round trip error / bound = %.3f\n", e, err / (2e-5 * (1 + scale))); return 1; }
    }
    bool threw = false;
    try { batch.inverseDynamics(nullptr, {}, nullptr, nullptr, false, nullptr, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("dynamics through the facade, %d envs: bit-identical to the C-ABI, round trip error / bound %.3f\n", N, worst);
    std::printf("dynamics_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
