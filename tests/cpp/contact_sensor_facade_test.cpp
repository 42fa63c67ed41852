// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::getBodyContactWrenches / getContactReadings / updateContactTimers
// (all envs in one call, computed on the device) against the loop they replace - per env, on the host, in double, over ArticulatedSystem::getContacts()
// with the body poses and velocities of the per-env view (getFramePosition / getFrameOrientation / getFrameVelocity / getFrameAngularVelocity).  The
// ANYmal-like model is dropped without joint control from a few heights, rolls and speeds, so several links per env touch; one env stays in the air.
//   force, torque, normal force, slip   |device - host| <= 2e-5 (1 + S), S the sum of the absolute terms of the host's expression
//   count                               equal
//   contact flag                        equal wherever the host's normal force is further than its bar from the threshold
//   columns 1..3 of the readings        the bits of the force; the timers follow their table in float
// Exit code 0 = all checks passed, 1 = a check failed or no device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/World.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
void cross(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
double norm(const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: contact_sensor_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 6;
    const double bar = 2e-5;
    const float threshold = 1.f;
    raisim::BatchedWorld batch(urdf, N);
    batch.addGround(0.0);
    batch.setTimeStep(0.0025);
    const int nq = batch.gcDim(), nv = batch.dof(), nb = batch.blob().nb;
    CHECK(nq == 19);
    const float joints[12] = {0.03f, 0.4f, -0.8f, -0.03f, 0.4f, -0.8f, 0.03f, -0.4f, 0.8f, -0.03f, -0.4f, 0.8f};
    std::vector<float> gc((size_t)N * nq, 0.f), gv((size_t)N * nv, 0.f);
    for (int e = 0; e < N; ++e) {
      float* q = gc.data() + (size_t)e * nq;
      q[0] = 0.7f * e; q[1] = -0.4f * e; q[2] = e == N - 1 ? 3.f : 0.45f + 0.03f * e;
      const float roll = 0.15f * e;      // the later envs come down on one side
      q[3] = std::cos(0.5f * roll); q[4] = std::sin(0.5f * roll);
      for (int k = 0; k < 12; ++k) q[7 + k] = joints[k] * (1.f + 0.1f * e);
      gv[(size_t)e * nv] = 0.3f * e;     // and slide
    }
    batch.setState(gc.data(), gv.data());
    batch.integrate(70);
    const double invDt = (double)(float)(1.0 / batch.getTimeStep());

    std::vector<rsb_frame> frames;
    for (int b = 0; b < nb; ++b) frames.push_back(rsb_frame{b, {0.f, 0.f, 0.f}});
    frames.push_back(rsb_frame{3, {0.02f, -0.01f, -0.3f}});
    frames.push_back(rsb_frame{0, {0.3f, 0.1f, -0.05f}});
    const int F = (int)frames.size();
    const size_t pairs = (size_t)N * F;
    std::vector<float> force(pairs * 3), torque(pairs * 3), forceL(pairs * 3), torqueL(pairs * 3), rows(pairs * 6), only(pairs * 3, 7.f);
    std::vector<int32_t> count(pairs);
    batch.getBodyContactWrenches(frames, false, true, force.data(), torque.data(), count.data());
    batch.getBodyContactWrenches(frames, true, true, forceL.data(), torqueL.data(), nullptr);
    batch.getBodyContactWrenches(frames, false, true, nullptr, only.data(), nullptr);
    CHECK(!std::memcmp(only.data(), torque.data(), only.size() * 4));
    batch.getContactReadings(frames, threshold, false, true, rows.data());

    int owned = 0, flags = 0, nearThreshold = 0, bodiesTouching = 0;
    double worst[4] = {0, 0, 0, 0};
    for (int e = 0; e < N; ++e) {
      raisim::World view(batch, e);
      raisim::ArticulatedSystem* robot = view.addArticulatedSystem(urdf);
      const std::vector<raisim::Contact>& contacts = robot->getContacts();
      if (e == N - 1) CHECK(contacts.empty());
      for (int f = 0; f < F; ++f) {
        const size_t body = (size_t)frames[f].body;
        raisim::Vec<3> p, v, w;
        raisim::Mat<3, 3> R;
        robot->getFramePosition(body, p); robot->getFrameOrientation(body, R); robot->getFrameVelocity(body, v); robot->getFrameAngularVelocity(body, w);
        double pf[3], spf[3], fo[3] = {0, 0, 0}, to[3] = {0, 0, 0}, sf[3] = {0, 0, 0}, st[3] = {0, 0, 0}, nf = 0, sn = 0, slip = 0, ss = 0;
        for (int r = 0; r < 3; ++r) {
          pf[r] = p[r]; spf[r] = std::fabs(p[r]);
          for (int c = 0; c < 3; ++c) { pf[r] += R(r, c) * frames[f].offset[c]; spf[r] += std::fabs(R(r, c) * frames[f].offset[c]); }
        }
        int n = 0;
        for (const raisim::Contact& con : contacts) {
          if (con.getlocalBodyIndex() != body) continue;
          const raisim::Vec<3> pos = con.getPosition(), nrm = con.getNormal(), imp = con.getImpulse();
          double fc[3], lever[3], t[3], ap[3], af[3], a1[3], a2[3], d[3], wd[3], vel[3];
          for (int k = 0; k < 3; ++k) { fc[k] = imp[k] * invDt; lever[k] = pos[k] - pf[k]; ap[k] = std::fabs(pos[k]); af[k] = std::fabs(fc[k]); d[k] = pos[k] - p[k]; }
          cross(lever, fc, t);
          const double m1[3] = {ap[1] * af[2] + ap[2] * af[1], ap[2] * af[0] + ap[0] * af[2], ap[0] * af[1] + ap[1] * af[0]};
          const double m2[3] = {spf[1] * af[2] + spf[2] * af[1], spf[2] * af[0] + spf[0] * af[2], spf[0] * af[1] + spf[1] * af[0]};
          for (int k = 0; k < 3; ++k) { fo[k] += fc[k]; sf[k] += af[k]; to[k] += t[k]; st[k] += m1[k] + m2[k]; a1[k] = v[k]; a2[k] = w[k]; }
          nf += (imp[0] * nrm[0] + imp[1] * nrm[1] + imp[2] * nrm[2]) * invDt;
          sn += (std::fabs(imp[0] * nrm[0]) + std::fabs(imp[1] * nrm[1]) + std::fabs(imp[2] * nrm[2])) * invDt;
          cross(a2, d, wd);
          for (int k = 0; k < 3; ++k) vel[k] = a1[k] + wd[k];
          const double vn = vel[0] * nrm[0] + vel[1] * nrm[1] + vel[2] * nrm[2];
          double tang[3], pp[3] = {p[0], p[1], p[2]}, pc[3] = {pos[0], pos[1], pos[2]};
          for (int k = 0; k < 3; ++k) tang[k] = vel[k] - vn * nrm[k];
          slip = std::max(slip, norm(tang));
          ss = std::max(ss, norm(a1) + norm(a2) * (norm(pc) + norm(pp)));
          ++n;
        }
        const size_t at = (size_t)e * F + f;
        CHECK(count[at] == n);
        owned += n;
        if (n && f < nb) ++bodiesTouching;
        for (int k = 0; k < 3; ++k) {
          worst[0] = std::max(worst[0], std::fabs(force[at * 3 + k] - fo[k]) / (bar * (1 + sf[k])));
          worst[1] = std::max(worst[1], std::fabs(torque[at * 3 + k] - to[k]) / (bar * (1 + st[k])));
          double fl = 0, tl = 0, sfl = 0, stl = 0;      // R^T x
          for (int r = 0; r < 3; ++r) { fl += R(r, k) * fo[r]; tl += R(r, k) * to[r]; sfl += std::fabs(R(r, k)) * sf[r]; stl += std::fabs(R(r, k)) * st[r]; }
          worst[0] = std::max(worst[0], std::fabs(forceL[at * 3 + k] - fl) / (bar * (1 + sfl)));
          worst[1] = std::max(worst[1], std::fabs(torqueL[at * 3 + k] - tl) / (bar * (1 + stl)));
        }
        const float* row = rows.data() + at * 6;
        CHECK(!std::memcmp(row + 1, &force[at * 3], 12));
        worst[2] = std::max(worst[2], std::fabs(row[4] - nf) / (bar * (1 + sn)));
        worst[3] = std::max(worst[3], std::fabs(row[5] - slip) / (bar * (1 + ss)));
        CHECK(row[0] == (row[4] > threshold ? 1.f : 0.f));
        if (std::fabs(nf - threshold) > bar * (1 + sn)) CHECK(row[0] == (nf > threshold ? 1.f : 0.f)); else ++nearThreshold;
        flags += row[0] == 1.f;
      }
    }
    std::printf("error / bar: force %.3f torque %.3f normal %.3f slip %.3f; %d owned records, %d contact flags, %d (env, body) pairs in contact, %d pairs near the threshold\n",
                worst[0], worst[1], worst[2], worst[3], owned, flags, bodiesTouching, nearThreshold);
    for (double x : worst) CHECK(x <= 1.0);
    CHECK(owned >= 8 && flags >= 4 && nearThreshold * 100 < (int)pairs);

    // the timers: two calls on the same contact list follow the table, in float
    const float dt = 0.02f;
    std::vector<float> air(pairs, 0.25f), ct(pairs, 0.5f), td(pairs, 7.f);
    std::vector<uint8_t> reset(N, 0);
    reset[1] = 1;
    batch.updateContactTimers(frames, threshold, dt, reset.data(), air.data(), ct.data(), td.data());
    for (int e = 0; e < N; ++e)
      for (int f = 0; f < F; ++f) {
        const size_t at = (size_t)e * F + f;
        const bool contact = rows[at * 6] == 1.f;
        CHECK(air[at] == (reset[e] || contact ? 0.f : 0.25f + dt));
        CHECK(ct[at] == (reset[e] || !contact ? 0.f : 0.5f + dt));
        CHECK(td[at] == (!reset[e] && contact ? 0.25f : 0.f));
      }
    bool threw = false;
    try { batch.updateContactTimers(frames, threshold, dt, nullptr, nullptr, nullptr, td.data()); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    std::printf("contact_sensor_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
