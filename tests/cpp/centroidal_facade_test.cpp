// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::getCentroidal / getCentroidalMomentumMatrices (all envs in one call,
// computed on the device) against the C-ABI they wrap - bit for bit - and against the per-env host accessors of ArticulatedSystem (getCOM,
// getLinearMomentum, getAngularMomentum, getKineticEnergy, getPotentialEnergy, getEnergy): a second formulation in double that shares no code with the
// oracle.  Bounds per env as in tests/test_gpu_centroidal.py, with M the total mass, v_max the largest body-COM speed and r_max the largest body-COM
// distance from the centre of mass:
//   com 1e-5 (1 + |c|)   com_vel 2e-5 (1 + v_max)   lin_mom 2e-5 M (1 + v_max)   ang_mom 2e-5 M (1 + v_max)(1 + r_max)   kinetic 4e-5 (1 + T)
//   potential 1e-5 M |g| (1 + |c|);  A gv against the host's momenta under the momentum bounds.
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
unsigned g_seed = 777u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
double norm3(const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: centroidal_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 21;      // two workgroups of 19 ANYmal envs, the second with a tail
    raisim::BatchedWorld batch(urdf, N);
    const rsb_model_blob& b = batch.blob();
    const int nq = batch.gcDim(), nv = batch.dof(), nb = b.nb;
    std::vector<std::unique_ptr<raisim::World>> views;
    std::vector<raisim::ArticulatedSystem*> robots;
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      robots.push_back(views.back()->addArticulatedSystem(urdf));
      raisim::VecDyn g(nq), v(nv);
      double q4[4], n2 = 0;
      for (double& x : q4) { x = 2 * uni() - 1; n2 += x * x; }
      g[0] = 4 * uni() - 2 + (e % 4 == 0 ? 50.0 : 0.0); g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 2 * uni() - 1;
      for (int k = 0; k < nv; ++k) v[k] = 4 * uni() - 2;
      robots.back()->setState(g, v);        // staged through the view: the batched calls below must see it
    }
    std::vector<float> com(N * 3), cv(N * 3), P(N * 3), L(N * 3), T(N), U(N), A((size_t)N * 6 * nv);
    batch.getCentroidal(com.data(), cv.data(), P.data(), L.data(), T.data(), U.data());
    batch.getCentroidalMomentumMatrices(A.data());
    // the facade's members are the C-ABI's calls: the same bits
    {
      std::vector<float> com2(N * 3), cv2(N * 3), P2(N * 3), L2(N * 3), T2(N), U2(N), A2(A.size());
      RSB_CHECK(rsb_get_centroidal(batch.handle(), com2.data(), cv2.data(), P2.data(), L2.data(), T2.data(), U2.data(), RSB_HOST));
      RSB_CHECK(rsb_get_centroidal_momentum_matrix(batch.handle(), A2.data(), RSB_HOST));
      CHECK(!std::memcmp(com.data(), com2.data(), com.size() * 4) && !std::memcmp(cv.data(), cv2.data(), cv.size() * 4) && !std::memcmp(P.data(), P2.data(), P.size() * 4));
      CHECK(!std::memcmp(L.data(), L2.data(), L.size() * 4) && !std::memcmp(T.data(), T2.data(), T.size() * 4) && !std::memcmp(U.data(), U2.data(), U.size() * 4));
      CHECK(!std::memcmp(A.data(), A2.data(), A.size() * 4));
      std::vector<float> only(N, 7.f);      // null outputs are skipped
      batch.getCentroidal(nullptr, nullptr, nullptr, nullptr, only.data(), nullptr);
      CHECK(!std::memcmp(only.data(), T.data(), only.size() * 4));
    }
    raisim::Vec<3> g;
    g[2] = -9.81;      // the world's default
    const double gn = 9.81, M = robots[0]->getTotalMass();
    double worst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < N; ++e) {
      raisim::ArticulatedSystem* r = robots[e];
      const raisim::Vec<3> c = r->getCOM();
      raisim::Vec<3> p, l;
      r->getLinearMomentum(p);
      r->getAngularMomentum(c, l);
      const double t = r->getKineticEnergy(), u = r->getPotentialEnergy(g);
      CHECK(std::fabs(r->getEnergy(g) - (t + u)) <= 1e-12 * (1 + std::fabs(t + u)));
      double vmax = 0, rmax = 0;
      for (int i = 0; i < nb; ++i) {
        raisim::Vec<3> cb, pw, vw;
        for (int k = 0; k < 3; ++k) cb[k] = b.com[i][k];
        r->getPosition(i, cb, pw);
        r->getVelocity(i, cb, vw);
        const double d[3] = {pw[0] - c[0], pw[1] - c[1], pw[2] - c[2]};
        vmax = std::max(vmax, norm3(vw.data())); rmax = std::max(rmax, norm3(d));
      }
      const double cn = norm3(c.data());
      const raisim::VecDyn& gv = r->getGeneralizedVelocity();
      double err[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < 3; ++k) {
        err[0] = std::max(err[0], std::fabs(com[e * 3 + k] - c[k]) / (1e-5 * (1 + cn)));
        err[1] = std::max(err[1], std::fabs(cv[e * 3 + k] - p[k] / M) / (2e-5 * (1 + vmax)));
        err[2] = std::max(err[2], std::fabs(P[e * 3 + k] - p[k]) / (2e-5 * M * (1 + vmax)));
        err[3] = std::max(err[3], std::fabs(L[e * 3 + k] - l[k]) / (2e-5 * M * (1 + vmax) * (1 + rmax)));
        double ap = 0, al = 0;
        for (int d = 0; d < nv; ++d) { ap += (double)A[((size_t)e * 6 + k) * nv + d] * gv[d]; al += (double)A[((size_t)e * 6 + 3 + k) * nv + d] * gv[d]; }
        err[6] = std::max(err[6], std::fabs(ap - p[k]) / (2e-5 * M * (1 + vmax)));
        err[7] = std::max(err[7], std::fabs(al - l[k]) / (2e-5 * M * (1 + vmax) * (1 + rmax)));
      }
      err[4] = std::fabs(T[e] - t) / (4e-5 * (1 + t));
      err[5] = std::fabs(U[e] - u) / (1e-5 * M * gn * (1 + cn));
      for (int i = 0; i < 8; ++i) worst[i] = std::max(worst[i], err[i]);
      for (int i = 0; i < 8; ++i) if (!(err[i] <= 1.0)) { std::printf("env %d quantity %d: error / bound = %.3f\n", e, i, err[i]); return 1; }
    }
    std::printf("centroidal vs per-env host accessors, %d envs, error / bound: com %.3f com_vel %.3f lin_mom %.3f ang_mom %.3f kinetic %.3f potential %.3f A gv lin %.3f ang %.3f\n",
                N, worst[0], worst[1], worst[2], worst[3], worst[4], worst[5], worst[6], worst[7]);
    std::printf("centroidal_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
