// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::getFrameKinematics / getFrameJacobians / addExternalWrench (all envs
// in one call, computed on the device) against the per-env host accessors of ArticulatedSystem (getFramePosition, getFrameOrientation,
// getFrameVelocity, getFrameAngularVelocity, getDenseFrameJacobian, getDenseFrameRotationalJacobian, setExternalForce, setExternalTorque): a second
// formulation in double that shares no code with the oracle.  Bounds as in tests/test_gpu_frames.py: 1e-5 (1 + max |ref|) per env for positions,
// orientations and Jacobians, 2e-5 (1 + max |ref|) for velocities and feed-forward rows.
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

// running max |dev - ref| and max |ref| of one env and quantity
struct Err {
  double err = 0, ref = 0;
  void add(double dev, double r) { err = std::max(err, std::fabs(dev - r)); ref = std::max(ref, std::fabs(r)); }
  bool within(double tol) const { return err <= tol * (1.0 + ref); }
  double rel() const { return err / (1.0 + ref); }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: frames_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 16;
    raisim::BatchedWorld batch(urdf, N), twin(urdf, N);
    const int nq = batch.gcDim(), nv = batch.dof(), nb = nv - 5;
    std::vector<std::unique_ptr<raisim::World>> views, tviews;
    std::vector<raisim::ArticulatedSystem*> robots, trobots;
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      robots.push_back(views.back()->addArticulatedSystem(urdf));
      tviews.push_back(std::make_unique<raisim::World>(twin, e));
      trobots.push_back(tviews.back()->addArticulatedSystem(urdf));
      raisim::VecDyn g(nq), v(nv);
      double q4[4], n2 = 0;
      for (double& x : q4) { x = 2 * uni() - 1; n2 += x * x; }
      g[0] = 4 * uni() - 2; g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 2 * uni() - 1;
      for (int k = 0; k < nv; ++k) v[k] = 2 * uni() - 1;
      robots.back()->setState(g, v);        // staged through the view: the batched calls below must see it
      trobots.back()->setState(g, v);
    }
    std::vector<rsb_frame> frames;
    for (int b = 0; b < nb; ++b) frames.push_back(rsb_frame{b, {0.f, 0.f, 0.f}});
    const size_t F = frames.size();
    std::vector<float> pos(N * F * 3), rot(N * F * 9), lin(N * F * 3), ang(N * F * 3), Jl(N * F * 3 * nv), Jr(N * F * 3 * nv);
    batch.getFrameKinematics(frames, pos.data(), rot.data(), lin.data(), ang.data());
    batch.getFrameJacobians(frames, Jl.data(), Jr.data());
    double worst[6] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < N; ++e) {
      Err ep, er, el, ea, ejl, ejr;
      for (size_t b = 0; b < F; ++b) {
        const size_t k = (size_t)e * F + b;
        raisim::Vec<3> p, v, w;
        raisim::Mat<3, 3> R;
        raisim::MatDyn J, Jrot;
        robots[e]->getFramePosition(b, p);
        robots[e]->getFrameOrientation(b, R);
        robots[e]->getFrameVelocity(b, v);
        robots[e]->getFrameAngularVelocity(b, w);
        robots[e]->getDenseFrameJacobian(b, J);
        robots[e]->getDenseFrameRotationalJacobian(b, Jrot);
        for (int c = 0; c < 3; ++c) { ep.add(pos[k * 3 + c], p[c]); el.add(lin[k * 3 + c], v[c]); ea.add(ang[k * 3 + c], w[c]); }
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) er.add(rot[k * 9 + 3 * r + c], R(r, c));
        for (int r = 0; r < 3; ++r) for (int d = 0; d < nv; ++d) { ejl.add(Jl[(k * 3 + r) * nv + d], J(r, d)); ejr.add(Jr[(k * 3 + r) * nv + d], Jrot(r, d)); }
      }
      const Err* all[6] = {&ep, &er, &ejl, &ejr, &el, &ea};
      for (int i = 0; i < 6; ++i) worst[i] = std::max(worst[i], all[i]->rel());
      CHECK(ep.within(1e-5)); CHECK(er.within(1e-5)); CHECK(ejl.within(1e-5)); CHECK(ejr.within(1e-5));
      CHECK(el.within(2e-5)); CHECK(ea.within(2e-5));
    }
    std::printf("frames vs per-env host accessors, %d envs x %zu bodies: pos %.2e rot %.2e J_lin %.2e J_rot %.2e lin_vel %.2e ang_vel %.2e\n", N, F, worst[0], worst[1],
                worst[2], worst[3], worst[4], worst[5]);
    // null outputs are skipped
    std::vector<float> pos2(pos.size(), 7.f);
    batch.getFrameKinematics(frames, pos2.data(), nullptr, nullptr, nullptr);
    CHECK(std::memcmp(pos2.data(), pos.data(), pos.size() * sizeof(float)) == 0);

    // addExternalWrench on a shank vs setExternalForce + setExternalTorque per env on the twin; every second env masked out
    const int body = nb - 1;
    std::vector<float> force(N * 3), torque(N * 3);
    std::vector<uint8_t> mask(N);
    for (int e = 0; e < N; ++e) {
      mask[e] = (uint8_t)(e % 2 == 0);
      raisim::Vec<3> f, t;
      for (int c = 0; c < 3; ++c) {
        force[e * 3 + c] = (float)(40 * uni() - 20); torque[e * 3 + c] = (float)(10 * uni() - 5);
        f[c] = force[e * 3 + c]; t[c] = torque[e * 3 + c];
      }
      if (mask[e]) { trobots[e]->setExternalForce(body, f); trobots[e]->setExternalTorque(body, t); }
    }
    batch.addExternalWrench(rsb_frame{body, {0.f, 0.f, 0.f}}, force.data(), torque.data(), mask.data());
    twin.uploadStaged();
    std::vector<float> ta((size_t)N * nv), tb((size_t)N * nv);
    RSB_CHECK(rsb_get_field(batch.handle(), RSB_F_TAU_FF, ta.data(), RSB_HOST));
    RSB_CHECK(rsb_get_field(twin.handle(), RSB_F_TAU_FF, tb.data(), RSB_HOST));
    double wt = 0;
    for (int e = 0; e < N; ++e) {
      Err et;
      bool any = false;
      for (int d = 0; d < nv; ++d) { et.add(ta[(size_t)e * nv + d], tb[(size_t)e * nv + d]); any = any || ta[(size_t)e * nv + d] != 0.f; }
      CHECK(et.within(2e-5));
      CHECK(any == (mask[e] != 0));
      wt = std::max(wt, et.rel());
    }
    // the per-env view reads the batched wrench back (its host mirror of the feed-forward rows is refetched) and clears it
    const std::vector<float> before = ta;
    robots[0]->clearExternalForces();
    batch.uploadStaged();
    RSB_CHECK(rsb_get_field(batch.handle(), RSB_F_TAU_FF, ta.data(), RSB_HOST));
    for (int d = 0; d < nv; ++d) CHECK(ta[d] == 0.f);
    CHECK(std::memcmp(ta.data() + nv, before.data() + nv, (size_t)(N - 1) * nv * sizeof(float)) == 0);      // the other envs keep theirs
    std::printf("frames_facade_test OK (tau_ff %.2e)\n", wt);
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
