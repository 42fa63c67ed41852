// CPU-tier test of the per-env whole-body accessors of raisim::ArticulatedSystem (getCOM, getLinearMomentum, getAngularMomentum, getKineticEnergy,
// getPotentialEnergy, getEnergy; include/raisim/World.hpp) against closed forms, through the C-ABI TEST DOUBLE (tests/cpp/rsb_host_double.cpp: it only
// has to hold the rows - the accessors compute on the host from the env's row and the model blob).
//   1. a free body with an off-centre centre of mass and three different principal inertias, rotated, translating and spinning:
//      com = p + R c, P = m v_c (v_c = v + w x R c), L_c = R I R^T w, T = 1/2 m v_c^2 + 1/2 w . R I R^T w, U = -m g . com, L_p = L_c + (com - p) x P
//   2. a revolute + prismatic arm rooted at `world` (fixed base), whose base entries of gv hold non-zero numbers that must be ignored.
// The closed forms are evaluated on the rows as the world holds them (float32), so the bound is double round-off: 1e-12 (1 + |ref|).
// usage: centroidal_host_test <scratch dir>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "raisim/World.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
bool close(double a, double b) { return std::fabs(a - b) <= 1e-12 * (1.0 + std::fabs(b)); }
bool close3(const raisim::Vec<3>& a, const double* b) { return close(a[0], b[0]) && close(a[1], b[1]) && close(a[2], b[2]); }
void cross(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

const char* kBody = R"(<?xml version="1.0"?>
<robot name="brick">
  <link name="brick">
    <inertial><origin xyz="0.03 -0.05 0.04"/><mass value="2.0"/><inertia ixx="0.01" ixy="0" ixz="0" iyy="0.02" iyz="0" izz="0.03"/></inertial>
    <collision><origin xyz="0 0 0"/><geometry><sphere radius="0.1"/></geometry></collision>
  </link>
</robot>
)";

const char* kArm = R"(<?xml version="1.0"?>
<robot name="arm">
  <link name="world"/>
  <link name="mount"><inertial><origin xyz="0 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial></link>
  <joint name="bolt" type="fixed"><origin xyz="0 0 0.5"/><parent link="world"/><child link="mount"/></joint>
  <link name="upper"><inertial><origin xyz="0.15 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial></link>
  <joint name="shoulder" type="revolute"><origin xyz="0 0 0"/><parent link="mount"/><child link="upper"/><axis xyz="0 0 1"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
  <link name="slider"><inertial><origin xyz="0.1 0 0"/><mass value="0.5"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial></link>
  <joint name="rail" type="prismatic"><origin xyz="0.3 0 0"/><parent link="upper"/><child link="slider"/><axis xyz="1 0 0"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
</robot>
)";

std::string write(const std::string& dir, const char* name, const char* text) {
  const std::string path = dir + "/" + name;
  std::ofstream(path) << text;
  return path;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: centroidal_host_test <scratch dir>\n"); return 2; }
  const std::string dir = argv[1];
  try {
    const raisim::Vec<3> g = [] { raisim::Vec<3> v; v[0] = 0.3; v[1] = -0.2; v[2] = -9.81; return v; }();
    {   // 1. the free body, env 1 of 3 (the other rows hold something else)
      const std::string urdf = write(dir, "brick.urdf", kBody);
      raisim::BatchedWorld batch(urdf, 3);
      raisim::World view(batch, 1);
      raisim::ArticulatedSystem* body = view.addArticulatedSystem(urdf);
      CHECK(!body->isFixedBase() && body->getDOF() == 6);
      raisim::VecDyn gc(7), gv(6);
      const double q0[7] = {1.25, -0.75, 2.5, 0.5, 0.5, -0.5, 0.5};      // a unit quaternion that float32 holds exactly
      const double u0[6] = {0.4, -1.1, 0.7, 1.3, -0.6, 0.9};
      for (int k = 0; k < 7; ++k) gc[k] = q0[k];
      for (int k = 0; k < 6; ++k) gv[k] = u0[k];
      body->setState(gc, gv);
      raisim::VecDyn q, u;
      body->getState(q, u);                                               // the row as the world holds it
      const double w = q[3], x = q[4], y = q[5], z = q[6];
      CHECK(w * w + x * x + y * y + z * z == 1.0);
      const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                           2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
      const double m = 2.0, c[3] = {0.03, -0.05, 0.04}, I[3] = {0.01, 0.02, 0.03};
      double Rc[3], com[3], om[3] = {u[3], u[4], u[5]}, wr[3], vc[3], P[3], wb[3], L[3];
      for (int r = 0; r < 3; ++r) { Rc[r] = R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]; com[r] = q[r] + Rc[r]; }
      cross(om, Rc, wr);
      for (int r = 0; r < 3; ++r) { vc[r] = u[r] + wr[r]; P[r] = m * vc[r]; }
      for (int k = 0; k < 3; ++k) wb[k] = R[k] * om[0] + R[3 + k] * om[1] + R[6 + k] * om[2];
      for (int r = 0; r < 3; ++r) L[r] = R[3 * r] * I[0] * wb[0] + R[3 * r + 1] * I[1] * wb[1] + R[3 * r + 2] * I[2] * wb[2];
      const double T = 0.5 * m * dot(vc, vc) + 0.5 * dot(om, L), U = -m * (g[0] * com[0] + g[1] * com[1] + g[2] * com[2]);
      raisim::Vec<3> got, ref;
      CHECK(close3(body->getCOM(), com));
      body->getLinearMomentum(got); CHECK(close3(got, P));
      body->getAngularMomentum(body->getCOM(), got); CHECK(close3(got, L));
      ref[0] = 0.5; ref[1] = 4.0; ref[2] = -1.0;
      double d[3] = {com[0] - ref[0], com[1] - ref[1], com[2] - ref[2]}, dxP[3], Lp[3];
      cross(d, P, dxP);
      for (int r = 0; r < 3; ++r) Lp[r] = L[r] + dxP[r];
      body->getAngularMomentum(ref, got); CHECK(close3(got, Lp));
      CHECK(close(body->getKineticEnergy(), T) && T > 1.0);
      CHECK(close(body->getPotentialEnergy(g), U));
      CHECK(close(body->getEnergy(g), T + U));
      CHECK(close(body->getTotalMass(), m));
    }
    {   // 2. the arm on a `world` root: joints only through the view, the base entries of gv set through the batch
      const std::string urdf = write(dir, "arm.urdf", kArm);
      raisim::BatchedWorld batch(urdf, 2);
      raisim::World view(batch, 1);
      raisim::ArticulatedSystem* arm = view.addArticulatedSystem(urdf);
      CHECK(arm->isFixedBase() && arm->getDOF() == 2 && batch.dof() == 8 && batch.gcDim() == 9);
      std::vector<float> gc(2 * 9, 0.f), gv(2 * 8, 0.f);
      for (int e = 0; e < 2; ++e) {
        gc[e * 9 + 3] = 1.f;
        for (int k = 0; k < 6; ++k) gv[e * 8 + k] = 0.5f + (float)k;     // must be ignored
      }
      gc[9 + 7] = 0.7f; gc[9 + 8] = 0.125f; gv[8 + 6] = -1.5f; gv[8 + 7] = 0.75f;
      batch.setState(gc.data(), gv.data());
      const double th = gc[9 + 7], dd = gc[9 + 8], thd = gv[8 + 6], ddd = gv[8 + 7], cs = std::cos(th), sn = std::sin(th);
      const double mass[3] = {1.0, 1.0, 0.5}, izz[3] = {1e-2, 1e-2, 1e-3};
      const double ci[3][3] = {{0, 0, 0.5}, {0.15 * cs, 0.15 * sn, 0.5}, {(0.4 + dd) * cs, (0.4 + dd) * sn, 0.5}};
      const double vi[3][3] = {{0, 0, 0}, {-0.15 * thd * sn, 0.15 * thd * cs, 0}, {-(0.4 + dd) * thd * sn + ddd * cs, (0.4 + dd) * thd * cs + ddd * sn, 0}};
      const double wz[3] = {0, thd, thd};
      double M = 0, com[3] = {0, 0, 0}, P[3] = {0, 0, 0}, L0[3] = {0, 0, 0}, T = 0;
      for (int i = 0; i < 3; ++i) {
        double cv[3];
        cross(ci[i], vi[i], cv);
        M += mass[i];
        for (int r = 0; r < 3; ++r) { com[r] += mass[i] * ci[i][r]; P[r] += mass[i] * vi[i][r]; L0[r] += mass[i] * cv[r]; }
        L0[2] += izz[i] * wz[i];
        T += 0.5 * mass[i] * dot(vi[i], vi[i]) + 0.5 * izz[i] * wz[i] * wz[i];
      }
      for (int r = 0; r < 3; ++r) com[r] /= M;
      double cP[3], Lc[3];
      cross(com, P, cP);
      for (int r = 0; r < 3; ++r) Lc[r] = L0[r] - cP[r];
      raisim::Vec<3> got, origin;
      CHECK(close3(arm->getCOM(), com));
      arm->getLinearMomentum(got); CHECK(close3(got, P));
      arm->getAngularMomentum(arm->getCOM(), got); CHECK(close3(got, Lc));
      arm->getAngularMomentum(origin, got); CHECK(close3(got, L0));
      CHECK(close(arm->getKineticEnergy(), T) && T > 0.1);
      CHECK(close(arm->getPotentialEnergy(g), -M * (g[0] * com[0] + g[1] * com[1] + g[2] * com[2])));
      CHECK(close(arm->getEnergy(g), T - M * (g[0] * com[0] + g[1] * com[1] + g[2] * com[2])));
    }
    std::printf("centroidal_host_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
