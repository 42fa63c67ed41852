// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::inverseKinematics (all envs in one call, computed on the device)
// against the C-ABI it wraps - bit for bit, on host buffers - with the state rows STAGED through per-env views, which the member has to upload
// first: a second world that was given the same rows through rsb_set_state answers with the same bits.  The targets are the four feet's positions
// at joint angles 0.1 rad away from the start (read from the second world), so every env converges; null outputs are skipped; a call without
// outputs throws.  The tight checks are tests/test_gpu_ik.py's.
// Exit code 0 = all checks passed, 1 = a check failed or no device.
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
unsigned g_seed = 777u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: ik_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 21;      // two workgroups of 16 envs at m = 12, the second with a tail
    raisim::BatchedWorld batch(urdf, N), twin(urdf, N);
    const int nq = batch.gcDim(), nv = batch.dof();
    std::vector<std::unique_ptr<raisim::World>> views;
    std::vector<float> gc((size_t)N * nq), gv((size_t)N * nv, 0.f), moved(gc.size());
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      raisim::ArticulatedSystem* robot = views.back()->addArticulatedSystem(urdf);
      raisim::VecDyn g(nq), v(nv);
      double q4[4], n2 = 0;
      for (double& x : q4) { x = 2 * uni() - 1; n2 += x * x; }
      g[0] = 4 * uni() - 2; g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 0.3 + 0.6 * uni();      // (knees bent)
      for (int k = 0; k < nv; ++k) v[k] = 0.0;
      robot->setState(g, v);        // staged through the view: the batched call below must see it
      for (int k = 0; k < nq; ++k) {
        gc[(size_t)e * nq + k] = (float)g[k];
        moved[(size_t)e * nq + k] = (float)g[k] + (k >= 7 ? (float)(0.2 * uni() - 0.1) : 0.f);
      }
    }
    const rsb_model_blob& blob = batch.blob();
    std::vector<rsb_frame> feet;      // the last body of each leg: bodies without children
    for (int b = 1; b < blob.nb; ++b) {
      bool leaf = true;
      for (int c = b + 1; c < blob.nb; ++c) leaf = leaf && blob.parent[c] != b;
      if (leaf) feet.push_back({b, {0.f, 0.f, -0.3f}});
    }
    CHECK(feet.size() == 4);
    const int F = 4;
    std::vector<float> target((size_t)N * F * 3);
    RSB_CHECK(rsb_set_state(twin.handle(), moved.data(), gv.data(), nullptr, RSB_HOST));
    RSB_CHECK(rsb_get_frame_kinematics(twin.handle(), feet.data(), F, target.data(), nullptr, nullptr, nullptr, RSB_HOST));
    RSB_CHECK(rsb_set_state(twin.handle(), gc.data(), gv.data(), nullptr, RSB_HOST));
    const rsb_ik_options opt{30, 1e-3f, 1e-4f, 1e-4f, 0.5f};
    std::vector<float> q1(gc.size(), 7.f), q2(gc.size(), 7.f), e1((size_t)N * 2, 7.f), e2(e1.size(), 7.f);
    std::vector<int32_t> i1(N, -1), i2(N, -1), s1(N, -1), s2(N, -1);
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.inverseKinematics(feet, target.data(), nullptr, nullptr, nullptr, false, opt, q1.data(), e1.data(), i1.data(), s1.data());
    RSB_CHECK(rsb_inverse_kinematics(twin.handle(), feet.data(), F, 0, target.data(), nullptr, nullptr, nullptr, &opt, q2.data(), e2.data(), i2.data(), s2.data(), RSB_HOST));
    CHECK(same(q1, q2) && same(e1, e2) && same(i1, i2) && same(s1, s2));
    for (int e = 0; e < N; ++e) {
      CHECK(s1[e] == RSB_IK_CONVERGED && i1[e] >= 1 && i1[e] <= 30 && e1[(size_t)e * 2] <= 1e-4f && e1[(size_t)e * 2 + 1] == 0.f);
      for (int k = 0; k < 7; ++k) CHECK(!std::memcmp(&q1[(size_t)e * nq + k], &gc[(size_t)e * nq + k], sizeof(float)));      // the base is held
    }
    // ... and the member is the C-ABI's call on the facade's own world: the same bits again, from an explicit start too
    RSB_CHECK(rsb_inverse_kinematics(batch.handle(), feet.data(), F, 0, target.data(), nullptr, gc.data(), nullptr, &opt, q2.data(), e2.data(), i2.data(), s2.data(), RSB_HOST));
    CHECK(same(q1, q2) && same(e1, e2) && same(i1, i2) && same(s1, s2));
    // null outputs are skipped
    std::vector<float> only(gc.size(), 7.f);
    batch.inverseKinematics(feet, target.data(), nullptr, nullptr, nullptr, false, opt, only.data(), nullptr, nullptr, nullptr);
    CHECK(same(only, q1));
    std::vector<int32_t> st(N, -1);
    batch.inverseKinematics(feet, target.data(), nullptr, nullptr, nullptr, false, opt, nullptr, nullptr, nullptr, st.data());
    CHECK(same(st, s1));
    // the result does what it says: the feet of the twin at q1 are at the targets within the tolerance and the frame-position bar
    std::vector<float> pos(target.size());
    RSB_CHECK(rsb_set_state(twin.handle(), q1.data(), gv.data(), nullptr, RSB_HOST));
    RSB_CHECK(rsb_get_frame_kinematics(twin.handle(), feet.data(), F, pos.data(), nullptr, nullptr, nullptr, RSB_HOST));
    double worst = 0;
    for (size_t k = 0; k < pos.size(); ++k) worst = std::fmax(worst, std::fabs((double)pos[k] - target[k]) / (1e-4 + 1e-5 * (1 + std::fabs((double)target[k]))));
    std::printf("feet at the result: largest |pos - target| / (pos_tol + 1e-5 (1 + |target|)) = %.3f\n", worst);
    CHECK(worst <= 1.5);
    bool threw = false;
    try { batch.inverseKinematics(feet, target.data(), nullptr, nullptr, nullptr, false, opt, nullptr, nullptr, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("inverse kinematics through the facade, %d envs: bit-identical to the C-ABI\n", N);
    std::printf("ik_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
