// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::getFrameAccelerations / getFrameJacobianRates / getImuReadings (all
// envs in one call, computed on the device) against the C-ABI they wrap - bit for bit, on host buffers - with the state rows STAGED through per-env
// views, which the batched members have to upload first: a second world that was given the same rows through rsb_set_state answers with the same
// bits.  With a second argument the state, the inputs and every result are written to that file (int32 N, nq, nv, F; then float32 gc, gv, udot,
// F x (body as int32, offset[3]), lin, ang (world), lin, ang (local, proper), Jdot_lin, Jdot_rot, imu [N,F,6]) for the Python path to be compared with.
// Exit code 0 = all checks passed, 1 = a check failed or no device.
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
unsigned g_seed = 777u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * 4); }
void put(std::FILE* f, const std::vector<float>& v) { std::fwrite(v.data(), 4, v.size(), f); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: frame_accel_facade_test <urdf> [dump file]\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 21;
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
      g[0] = 4 * uni() - 2; g[1] = 4 * uni() - 2; g[2] = 0.3 + uni();
      for (int k = 0; k < 4; ++k) g[3 + k] = q4[k] / std::sqrt(n2);
      for (int k = 7; k < nq; ++k) g[k] = 2 * uni() - 1;
      for (int k = 0; k < nv; ++k) v[k] = 4 * uni() - 2;
      robot->setState(g, v);        // staged through the view: the batched calls below must see it
      for (int k = 0; k < nq; ++k) gc[(size_t)e * nq + k] = (float)g[k];
      for (int k = 0; k < nv; ++k) gv[(size_t)e * nv + k] = (float)v[k];
    }
    RSB_CHECK(rsb_set_state(twin.handle(), gc.data(), gv.data(), nullptr, RSB_HOST));
    const std::vector<rsb_frame> frames = {{0, {0.1f, 0.f, 0.05f}}, {nb - 1, {0.05f, -0.02f, 0.1f}}, {nb / 2, {0.f, 0.04f, -0.06f}}, {nb - 1, {0.f, 0.f, 0.f}}};
    const int F = (int)frames.size();
    std::vector<float> udot((size_t)N * nv);
    for (float& x : udot) x = (float)(4 * uni() - 2);
    const size_t a3 = (size_t)N * F * 3, jn = a3 * nv, w6 = (size_t)N * F * 6;
    std::vector<float> l1(a3), a1(a3), ll1(a3), al1(a3), jl1(jn), jr1(jn), imu1(w6), l2(a3), a2(a3), jl2(jn), jr2(jn), imu2(w6);
    // the first batched call uploads the staged rows; the twin holds them through the C-ABI
    batch.getFrameAccelerations(frames, udot.data(), false, false, l1.data(), a1.data());
    RSB_CHECK(rsb_get_frame_accelerations(twin.handle(), frames.data(), F, udot.data(), 0, l2.data(), a2.data(), RSB_HOST));
    CHECK(same(l1, l2) && same(a1, a2));
    batch.getFrameAccelerations(frames, udot.data(), true, true, ll1.data(), al1.data());
    RSB_CHECK(rsb_get_frame_accelerations(twin.handle(), frames.data(), F, udot.data(), RSB_ACC_LOCAL | RSB_ACC_PROPER, l2.data(), a2.data(), RSB_HOST));
    CHECK(same(ll1, l2) && same(al1, a2) && !same(ll1, l1));
    batch.getFrameJacobianRates(frames, jl1.data(), jr1.data());
    RSB_CHECK(rsb_get_frame_jacobian_rates(twin.handle(), frames.data(), F, jl2.data(), jr2.data(), RSB_HOST));
    CHECK(same(jl1, jl2) && same(jr1, jr2));
    batch.getImuReadings(frames, udot.data(), imu1.data());
    RSB_CHECK(rsb_imu_observe(twin.handle(), frames.data(), F, udot.data(), imu2.data(), 0, RSB_HOST));
    CHECK(same(imu1, imu2));
    for (size_t p = 0; p < (size_t)N * F; ++p)      // the accelerometer columns ARE the local proper acceleration
      CHECK(!std::memcmp(&imu1[p * 6], &ll1[p * 3], 12));
    // a row stride leaves the other columns of a row alone; null outputs are skipped; no udot is a valid call
    const long long stride = 6 * F + 5;
    std::vector<float> wide((size_t)N * stride, 7.f), only(a3, 7.f);
    batch.getImuReadings(frames, udot.data(), wide.data(), stride);
    for (int e = 0; e < N; ++e) {
      CHECK(!std::memcmp(&wide[(size_t)e * stride], &imu1[(size_t)e * 6 * F], (size_t)6 * F * 4));
      for (int k = 6 * F; k < stride; ++k) CHECK(wide[(size_t)e * stride + k] == 7.f);
    }
    batch.getFrameAccelerations(frames, udot.data(), false, false, nullptr, only.data());
    CHECK(same(only, a1));
    batch.getFrameAccelerations(frames, nullptr, false, false, l2.data(), nullptr);
    CHECK(!same(l2, l1));
    bool threw = false;
    try { batch.getFrameJacobianRates(frames, nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    if (argc > 2) {
      std::FILE* f = std::fopen(argv[2], "wb");
      CHECK(f != nullptr);
      const int32_t head[4] = {N, nq, nv, F};
      std::fwrite(head, 4, 4, f);
      put(f, gc); put(f, gv); put(f, udot);
      for (const rsb_frame& fr : frames) { std::fwrite(&fr.body, 4, 1, f); std::fwrite(fr.offset, 4, 3, f); }
      put(f, l1); put(f, a1); put(f, ll1); put(f, al1); put(f, jl1); put(f, jr1); put(f, imu1);
      std::fclose(f);
    }
    std::printf("frame accelerations, Jacobian rates and IMU rows through the facade, %d envs x %d frames: bit-identical to the C-ABI\n", N, F);
    std::printf("frame_accel_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
