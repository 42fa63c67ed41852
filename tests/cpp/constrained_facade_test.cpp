// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::constrainedForwardDynamics / getFrameImpulse (all envs in one call,
// computed on the device) against the C-ABI they wrap - bit for bit, on host buffers - with the state rows STAGED through per-env views, which the
// batched members have to upload first: a second world that was given the same rows through rsb_set_state answers with the same bits.  Null outputs
// are skipped, every env of the four feet's linear rows is solved, the feet's six rows each are dependent without damping (status 1, lambda zero,
// udot the bits of forwardDynamics) and solved with it, and the held feet do not accelerate: getFrameAccelerations(udot) is zero within
// 2e-5 (1 + the largest |lambda| + the largest free acceleration), a loose sanity bound - the tight one is tests/test_gpu_constrained.py's.
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
template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: constrained_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 21;      // two workgroups of 16 envs at m = 12, the second with a tail
    raisim::BatchedWorld batch(urdf, N), twin(urdf, N);
    const int nq = batch.gcDim(), nv = batch.dof();
    std::vector<std::unique_ptr<raisim::World>> views;
    std::vector<float> gc((size_t)N * nq), gv((size_t)N * nv);
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      raisim::ArticulatedSystem* robot = views.back()->addArticulatedSystem(urdf);
      raisim::VecDyn g(nq), v(nv);
      double q4[4], n2 = 0;
      for (double& x : q4) { x = 2 * uni() - 1; n2 += x * x; }
      g[0] = 4 * uni() - 2; g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 0.3 + 0.6 * uni();      // (knees bent: the four feet's twelve linear rows are independent)
      for (int k = 0; k < nv; ++k) v[k] = 2 * uni() - 1;
      robot->setState(g, v);        // staged through the view: the batched calls below must see it
      for (int k = 0; k < nq; ++k) gc[(size_t)e * nq + k] = (float)g[k];
      for (int k = 0; k < nv; ++k) gv[(size_t)e * nv + k] = (float)v[k];
    }
    RSB_CHECK(rsb_set_state(twin.handle(), gc.data(), gv.data(), nullptr, RSB_HOST));
    const rsb_model_blob& blob = batch.blob();
    std::vector<rsb_frame> feet;      // the last body of each leg: bodies without children
    for (int b = 1; b < blob.nb; ++b) {
      bool leaf = true;
      for (int c = b + 1; c < blob.nb; ++c) leaf = leaf && blob.parent[c] != b;
      if (leaf) feet.push_back({b, {0.f, 0.f, -0.3f}});
    }
    CHECK(feet.size() == 4);
    const int F = 4, m = 3 * F;
    std::vector<float> tau((size_t)N * nv), diag(nv, 0.f), target((size_t)N * m);
    for (float& x : tau) x = (float)(10 * uni() - 5);
    for (float& x : target) x = (float)(2 * uni() - 1);
    for (int k = 6; k < nv; ++k) diag[k] = (float)(0.5 * uni());
    std::vector<float> u1((size_t)N * nv), u2(u1.size()), l1((size_t)N * m), l2(l1.size()), d1(u1.size()), d2(u1.size()), i1(l1.size()), i2(l1.size());
    std::vector<int32_t> s1(N, -1), s2(N, -1), t1(N, -1), t2(N, -1);
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.constrainedForwardDynamics(tau.data(), feet, false, target.data(), 0.f, u1.data(), l1.data(), s1.data());
    RSB_CHECK(rsb_constrained_forward_dynamics(twin.handle(), tau.data(), feet.data(), F, 0, target.data(), 0.f, u2.data(), l2.data(), s2.data(), RSB_HOST));
    CHECK(same(u1, u2) && same(l1, l2) && same(s1, s2));
    batch.getFrameImpulse(feet, false, target.data(), diag.data(), 0.f, d1.data(), i1.data(), t1.data());
    RSB_CHECK(rsb_frame_impulse(twin.handle(), feet.data(), F, 0, target.data(), diag.data(), 0.f, d2.data(), i2.data(), t2.data(), RSB_HOST));
    CHECK(same(d1, d2) && same(i1, i2) && same(t1, t2));
    for (int e = 0; e < N; ++e) CHECK(s1[e] == RSB_HELD_SOLVED && t1[e] == RSB_HELD_SOLVED);
    // ... and the members are the C-ABI's calls on the facade's own world: the same bits again
    RSB_CHECK(rsb_constrained_forward_dynamics(batch.handle(), tau.data(), feet.data(), F, 0, target.data(), 0.f, u2.data(), l2.data(), s2.data(), RSB_HOST));
    RSB_CHECK(rsb_frame_impulse(batch.handle(), feet.data(), F, 0, target.data(), diag.data(), 0.f, d2.data(), i2.data(), t2.data(), RSB_HOST));
    CHECK(same(u1, u2) && same(l1, l2) && same(s1, s2) && same(d1, d2) && same(i1, i2) && same(t1, t2));
    // null outputs are skipped
    std::vector<float> only(l1.size(), 7.f);
    batch.constrainedForwardDynamics(tau.data(), feet, false, target.data(), 0.f, nullptr, only.data(), nullptr);
    CHECK(same(only, l1));
    std::fill(only.begin(), only.end(), 7.f);
    batch.getFrameImpulse(feet, false, target.data(), diag.data(), 0.f, nullptr, only.data(), nullptr);
    CHECK(same(only, i1));
    // the feet held: their accelerations under udot vanish
    batch.constrainedForwardDynamics(tau.data(), feet, false, nullptr, 0.f, u1.data(), l1.data(), s1.data());
    std::vector<float> free_u(u1.size()), acc((size_t)N * F * 3), acc_free(acc.size());
    batch.forwardDynamics(tau.data(), {}, nullptr, nullptr, false, free_u.data());
    batch.getFrameAccelerations(feet, u1.data(), false, false, acc.data(), nullptr);
    batch.getFrameAccelerations(feet, free_u.data(), false, false, acc_free.data(), nullptr);
    double worst = 0;
    for (int e = 0; e < N; ++e) {
      double scale = 0, err = 0;
      for (int k = 0; k < m; ++k) {
        scale = std::max({scale, std::fabs((double)l1[(size_t)e * m + k]), std::fabs((double)acc_free[(size_t)e * m + k])});
        err = std::max(err, std::fabs((double)acc[(size_t)e * m + k]));
      }
      worst = std::max(worst, err / (2e-5 * (1 + scale)));
    }
    std::printf("held feet: largest |acceleration| / (2e-5 (1 + scale)) = %.3f\n", worst);
    CHECK(worst <= 50.0);
    // six rows per foot: dependent on the quadruped without damping, solved with it
    const int m6 = 6 * F;
    std::vector<float> l6((size_t)N * m6, 7.f);
    batch.constrainedForwardDynamics(tau.data(), feet, true, nullptr, 0.f, u2.data(), l6.data(), s2.data());
    for (int e = 0; e < N; ++e) CHECK(s2[e] == RSB_HELD_SINGULAR);
    for (float x : l6) CHECK(x == 0.f);
    CHECK(same(u2, free_u));
    batch.constrainedForwardDynamics(tau.data(), feet, true, nullptr, 1e-4f, u2.data(), l6.data(), s2.data());
    for (int e = 0; e < N; ++e) CHECK(s2[e] == RSB_HELD_SOLVED);
    bool threw = false;
    try { batch.constrainedForwardDynamics(tau.data(), feet, false, nullptr, 0.f, nullptr, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { batch.getFrameImpulse(feet, false, nullptr, nullptr, -1.f, d1.data(), nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("constrained dynamics through the facade, %d envs: bit-identical to the C-ABI\n", N);
    std::printf("constrained_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
