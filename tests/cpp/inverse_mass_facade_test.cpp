// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::applyInverseMass / getFrameDelassus (all envs in one call, computed on
// the device) against the C-ABI they wrap - bit for bit, on host buffers - with the state rows STAGED through per-env views, which the batched members
// have to upload first: a second world that was given the same rows through rsb_set_state answers with the same bits.  X in place has the bits of X out
// of place, G equals its transpose bit for bit, null outputs are skipped, and M X = B within 2e-5 (1 + the largest row of |M||X| + |B|) with M from
// getMassMatrices.
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
unsigned g_seed = 9191u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * 4); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: inverse_mass_facade_test <urdf>\n"); return 2; }
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
    const int F = (int)frames.size(), R = 3, K = 6 * F;
    std::vector<float> B((size_t)N * R * nv), diag(nv, 0.f);
    for (float& x : B) x = (float)(4 * uni() - 2);
    for (int k = 6; k < nv; ++k) diag[k] = (float)(0.5 * uni());
    std::vector<float> x1(B.size()), x2(B.size()), g1((size_t)N * K * K), g2(g1.size()), j1((size_t)N * K * nv), j2(j1.size());
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.applyInverseMass(B.data(), R, diag.data(), x1.data());
    RSB_CHECK(rsb_apply_inverse_mass(twin.handle(), B.data(), R, diag.data(), x2.data(), RSB_HOST));
    CHECK(same(x1, x2));
    batch.getFrameDelassus(frames, true, diag.data(), g1.data(), j1.data());
    RSB_CHECK(rsb_get_frame_delassus(twin.handle(), frames.data(), F, RSB_DELASSUS_ANGULAR, diag.data(), g2.data(), j2.data(), RSB_HOST));
    CHECK(same(g1, g2) && same(j1, j2));
    // ... and the members are the C-ABI's calls on the facade's own world: the same bits again
    RSB_CHECK(rsb_apply_inverse_mass(batch.handle(), B.data(), R, diag.data(), x2.data(), RSB_HOST));
    RSB_CHECK(rsb_get_frame_delassus(batch.handle(), frames.data(), F, RSB_DELASSUS_ANGULAR, diag.data(), g2.data(), j2.data(), RSB_HOST));
    CHECK(same(x1, x2) && same(g1, g2) && same(j1, j2));
    // in place; null outputs are skipped; no joint_diag is a valid call; G is its own transpose
    x2 = B;
    batch.applyInverseMass(x2.data(), R, diag.data(), x2.data());
    CHECK(same(x1, x2));
    std::vector<float> only(g1.size(), 7.f);
    batch.getFrameDelassus(frames, true, diag.data(), only.data(), nullptr);
    CHECK(same(only, g1));
    for (int e = 0; e < N; ++e)
      for (int i = 0; i < K; ++i)
        for (int j = 0; j < i; ++j) CHECK(g1[((size_t)e * K + i) * K + j] == g1[((size_t)e * K + j) * K + i]);
    // M X = B, conditioning-free
    batch.applyInverseMass(B.data(), R, nullptr, x1.data());
    std::vector<float> M((size_t)N * nv * nv);
    batch.integrate1();
    batch.getMassMatrices(M.data());
    double worst = 0;
    for (int e = 0; e < N; ++e)
      for (int r = 0; r < R; ++r) {
        const float* x = &x1[((size_t)e * R + r) * nv];
        const float* b = &B[((size_t)e * R + r) * nv];
        double scale = 0, err = 0;
        for (int i = 0; i < nv; ++i) {
          double s = 0, a = 0;
          for (int k = 0; k < nv; ++k) { const double m = M[((size_t)e * nv + i) * nv + k]; s += m * x[k]; a += std::fabs(m) * std::fabs((double)x[k]); }
          scale = std::max(scale, a + std::fabs((double)b[i]));
          err = std::max(err, std::fabs(s - b[i]));
        }
        worst = std::max(worst, err / (2e-5 * (1 + scale)));
        if (!(err <= 2e-5 * (1 + scale))) { std::printf("env %d column %d: residual / bound = %.3f\n", e, r, err / (2e-5 * (1 + scale))); return 1; }
      }
    bool threw = false;
    try { batch.getFrameDelassus(frames, false, nullptr, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { batch.applyInverseMass(B.data(), 0, nullptr, x1.data()); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("inverse mass through the facade, %d envs: bit-identical to the C-ABI, residual / bound %.3f\n", N, worst);
    std::printf("inverse_mass_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
