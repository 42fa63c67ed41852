// The per-env host loop behind tools/bench_frames.py: what the frame kinematics of every env cost through the per-env ArticulatedSystem accessors
// (getFramePosition, getFrameOrientation, getFrameVelocity, getFrameAngularVelocity; host forward kinematics in double, one env and one frame per
// call) - the only way to get them before BatchedWorld::getFrameKinematics.  usage: bench_frames_host <urdf> <num_envs> <frame>...   (frame = body index)
// Prints the median wall time of 3 passes over all envs and frames, in ms, and the batched call's wall time through the facade for scale.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/World.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::printf("usage: bench_frames_host <urdf> <num_envs> <body>...\n"); return 2; }
  try {
    const std::string urdf = argv[1];
    const int N = std::atoi(argv[2]);
    std::vector<size_t> bodies;
    for (int k = 3; k < argc; ++k) bodies.push_back((size_t)std::atoi(argv[k]));
    raisim::BatchedWorld batch(urdf, N);
    std::vector<std::unique_ptr<raisim::World>> views;
    std::vector<raisim::ArticulatedSystem*> robots;
    for (int e = 0; e < N; ++e) {
      views.push_back(std::make_unique<raisim::World>(batch, e));
      robots.push_back(views.back()->addArticulatedSystem(urdf));
    }
    using clk = std::chrono::steady_clock;
    double sink = 0;
    std::vector<double> ms;
    for (int pass = 0; pass < 4; ++pass) {      // (pass 0 warms the host mirrors of gc / gv up)
      const auto t0 = clk::now();
      for (int e = 0; e < N; ++e)
        for (size_t b : bodies) {
          raisim::Vec<3> p, v, w;
          raisim::Mat<3, 3> R;
          robots[e]->getFramePosition(b, p);
          robots[e]->getFrameOrientation(b, R);
          robots[e]->getFrameVelocity(b, v);
          robots[e]->getFrameAngularVelocity(b, w);
          sink += p[0] + R(0, 0) + v[0] + w[0];
        }
      if (pass) ms.push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::vector<rsb_frame> frames;
    for (size_t b : bodies) frames.push_back(rsb_frame{(int32_t)b, {0.f, 0.f, 0.f}});
    const size_t F = frames.size();
    std::vector<float> pos(N * F * 3), rot(N * F * 9), lin(N * F * 3), ang(N * F * 3);
    std::vector<double> bms;
    for (int pass = 0; pass < 4; ++pass) {
      const auto t0 = clk::now();
      batch.getFrameKinematics(frames, pos.data(), rot.data(), lin.data(), ang.data());
      if (pass) bms.push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
    }
    std::sort(bms.begin(), bms.end());
    std::printf("host_loop_ms %.3f batched_host_copy_ms %.3f envs %d frames %zu sink %.3f\n", ms[1], bms[1], N, F, sink);
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
