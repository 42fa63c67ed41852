// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::inverseDynamicsDerivatives / forwardDynamicsDerivatives (all envs in
// one call, computed on the device) against the C-ABI they wrap - bit for bit, on host buffers - with the state rows STAGED through per-env views, which
// the batched members have to upload first: a second world that was given the same rows through rsb_set_state answers with the same bits.  The product
// M dUdotDq = -dTauDq (taken at the udot the forward call returned) closes within 2e-4 (1 + the sum of the absolute terms of the product).
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
  if (argc < 2) { std::printf("usage: dynamics_derivatives_facade_test <urdf>\n"); return 2; }
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
    const size_t nn = (size_t)N * nv * nv;
    std::vector<float> q1(nn), v1(nn), a1(nn), q2(nn), v2(nn), a2(nn), u1((size_t)N * nv), u2(u1.size()), fq1(nn), fv1(nn), ft1(nn), fq2(nn), fv2(nn), ft2(nn);
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.inverseDynamicsDerivatives(udot.data(), frames, force.data(), torque.data(), q1.data(), v1.data(), a1.data());
    RSB_CHECK(rsb_inverse_dynamics_derivatives(twin.handle(), udot.data(), frames.data(), F, force.data(), torque.data(), 0, q2.data(), v2.data(), a2.data(), RSB_HOST));
    CHECK(same(q1, q2) && same(v1, v2) && same(a1, a2));
    batch.forwardDynamicsDerivatives(tau.data(), frames, force.data(), torque.data(), u1.data(), fq1.data(), fv1.data(), ft1.data());
    RSB_CHECK(rsb_forward_dynamics_derivatives(twin.handle(), tau.data(), frames.data(), F, force.data(), torque.data(), 0, u2.data(), fq2.data(), fv2.data(), ft2.data(),
                                               RSB_HOST));
    CHECK(same(u1, u2) && same(fq1, fq2) && same(fv1, fv2) && same(ft1, ft2));
    // ... and the members are the C-ABI's calls on the facade's own world: the same bits again
    RSB_CHECK(rsb_inverse_dynamics_derivatives(batch.handle(), udot.data(), frames.data(), F, force.data(), torque.data(), 0, q2.data(), v2.data(), a2.data(), RSB_HOST));
    RSB_CHECK(rsb_forward_dynamics_derivatives(batch.handle(), tau.data(), frames.data(), F, force.data(), torque.data(), 0, u2.data(), fq2.data(), fv2.data(), ft2.data(),
                                               RSB_HOST));
    CHECK(same(q1, q2) && same(v1, v2) && same(a1, a2) && same(u1, u2) && same(fq1, fq2) && same(fv1, fv2) && same(ft1, ft2));
    // null outputs are skipped; no loads and no udot are valid calls; the forward call's udot is forwardDynamics'
    std::vector<float> only(nn, 7.f), h1(nn), h2(nn);
    batch.inverseDynamicsDerivatives(udot.data(), frames, force.data(), torque.data(), nullptr, only.data(), nullptr);
    CHECK(same(only, v1));
    batch.forwardDynamicsDerivatives(tau.data(), frames, force.data(), torque.data(), nullptr, only.data(), nullptr, nullptr);
    CHECK(same(only, fq1));
    batch.inverseDynamicsDerivatives(nullptr, {}, nullptr, nullptr, h1.data(), nullptr, nullptr);
    RSB_CHECK(rsb_inverse_dynamics_derivatives(batch.handle(), nullptr, nullptr, 0, nullptr, nullptr, 0, h2.data(), nullptr, nullptr, RSB_HOST));
    CHECK(same(h1, h2));
    batch.forwardDynamics(tau.data(), frames, force.data(), torque.data(), false, u2.data());
    CHECK(same(u1, u2));
    // M dUdotDq + dTauDq = 0 at the udot the forward call returned
    batch.inverseDynamicsDerivatives(u1.data(), frames, force.data(), torque.data(), q2.data(), nullptr, a2.data());
    double worst = 0;
    for (int e = 0; e < N; ++e)
      for (int i = 0; i < nv; ++i)
        for (int j = 0; j < nv; ++j) {
          double sum = q2[((size_t)e * nv + i) * nv + j], mag = std::fabs(sum);
          for (int k = 0; k < nv; ++k) {
            const double t = (double)a2[((size_t)e * nv + i) * nv + k] * fq1[((size_t)e * nv + k) * nv + j];
            sum += t; mag += std::fabs(t);
          }
          worst = std::max(worst, std::fabs(sum) / (2e-4 * (1 + mag)));
        }
    if (!(worst <= 1.0)) { std::printf("M dUdotDq + dTauDq: residual / bound = %.3f\n", worst); return 1; }
    bool threw = false;
    try { batch.inverseDynamicsDerivatives(nullptr, {}, nullptr, nullptr, nullptr, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("dynamics derivatives through the facade, %d envs: bit-identical to the C-ABI, M dUdotDq + dTauDq residual / bound %.3f\n", N, worst);
    std::printf("dynamics_derivatives_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
