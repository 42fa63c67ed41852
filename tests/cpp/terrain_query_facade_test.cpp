// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::getTerrainHeights / heightScan / rayTest (all envs in one call,
// computed on the device) against HeightMap::getHeight, the facade's own host formulation of the surface in double: heights at random points,
// the world-aligned scan under the base (whose position is the state's), and rays straight down (distance = z - height).
// Bounds as in tests/test_gpu_terrain_query.py: 1e-5 (1 + max |ref|) for heights and distances, 4e-5 (1 + max(|p|, |pattern|)) for the scan.
// Exit code 0 = all checks passed, 1 = a check failed or no device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/World.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
unsigned g_seed = 777u;
double uni() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }      // [0, 1)
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: terrain_query_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 8, xs = 9, ys = 7, P = 37;
    const double xSize = 4.0, ySize = 3.0, cx = 0.5, cy = -0.25;
    raisim::BatchedWorld batch(urdf, N);
    std::vector<double> h(xs * ys);
    for (double& v : h) v = (float)(0.4 * uni() - 0.2);
    batch.addHeightMap(xs, ys, xSize, ySize, cx, cy, h);
    raisim::HeightMap hm(&batch, xs, ys, xSize, ySize, cx, cy, h);
    const int nq = batch.gcDim(), nv = batch.dof();
    std::vector<float> gc((size_t)N * nq, 0.f), gv((size_t)N * nv, 0.f);
    for (int e = 0; e < N; ++e) {
      float* q = gc.data() + (size_t)e * nq;
      q[0] = (float)(3 * uni() - 1); q[1] = (float)(2 * uni() - 1.25); q[2] = (float)(0.5 + 0.3 * uni());
      const double yaw = 6.283185307179586 * uni();
      q[3] = (float)std::cos(0.5 * yaw); q[6] = (float)std::sin(0.5 * yaw);
    }
    batch.setState(gc.data(), gv.data());

    // heights (a margin of 1 m around the footprint is queried too: the clamped region)
    std::vector<float> xy((size_t)N * P * 2), height((size_t)N * P), normal((size_t)N * P * 3);
    for (size_t k = 0; k < xy.size(); k += 2) { xy[k] = (float)(cx + (xSize + 2) * (uni() - 0.5)); xy[k + 1] = (float)(cy + (ySize + 2) * (uni() - 0.5)); }
    batch.getTerrainHeights(xy.data(), P, height.data(), normal.data());
    double worst = 0;
    for (size_t k = 0; k < height.size(); ++k) {
      const double ref = hm.getHeight(xy[2 * k], xy[2 * k + 1]);
      worst = std::max(worst, std::fabs(height[k] - ref) / (1.0 + std::fabs(ref)));
      const float* n = normal.data() + 3 * k;
      CHECK(std::fabs(std::sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]) - 1.0) <= 1e-5 && n[2] > 0.f);
    }
    std::printf("heights: max |dev - ref| / (1 + |ref|) = %.3g\n", worst);
    CHECK(worst <= 1e-5);

    // the world-aligned scan under the base, into the tail columns of wider rows
    const int head = 3;
    std::vector<float> pattern((size_t)P * 2), rowsOut((size_t)N * (head + P), 7.f);
    for (float& v : pattern) v = (float)(1.6 * uni() - 0.8);
    const std::vector<rsb_frame> base{rsb_frame{0, {0.f, 0.f, 0.f}}};
    batch.heightScan(base, pattern.data(), P, false, rowsOut.data() + head, head + P);
    worst = 0;
    for (int e = 0; e < N; ++e) {
      const float* q = gc.data() + (size_t)e * nq;
      const double scale = 1.0 + std::max({std::fabs((double)q[0]), std::fabs((double)q[1]), std::fabs((double)q[2]), 0.8});
      for (int c = 0; c < head; ++c) CHECK(rowsOut[(size_t)e * (head + P) + c] == 7.f);
      for (int k = 0; k < P; ++k) {
        const double ref = q[2] - hm.getHeight((double)q[0] + pattern[2 * k], (double)q[1] + pattern[2 * k + 1]);
        worst = std::max(worst, std::fabs(rowsOut[(size_t)e * (head + P) + head + k] - ref) / scale);
      }
    }
    std::printf("scan: max |dev - ref| / (1 + max(|p|, |pattern|)) = %.3g\n", worst);
    CHECK(worst <= 4e-5);
    // yaw-aligned: a different scan (the headings are random), same column discipline
    std::vector<float> yawOut((size_t)N * P);
    batch.heightScan(base, pattern.data(), P, true, yawOut.data());
    bool differs = false;
    for (int e = 0; e < N; ++e)
      for (int k = 0; k < P; ++k) differs = differs || yawOut[(size_t)e * P + k] != rowsOut[(size_t)e * (head + P) + head + k];
    CHECK(differs);

    // rays straight down from above the points queried first; one ray upwards misses
    std::vector<float> org((size_t)N * P * 3), dir((size_t)N * P * 3), dist((size_t)N * P);
    for (size_t k = 0; k < dist.size(); ++k) {
      org[3 * k] = (float)(cx + (xSize - 0.01) * (uni() - 0.5)); org[3 * k + 1] = (float)(cy + (ySize - 0.01) * (uni() - 0.5)); org[3 * k + 2] = (float)(0.5 + uni());
      dir[3 * k] = 0.f; dir[3 * k + 1] = 0.f; dir[3 * k + 2] = (float)(-0.5 - 2 * uni());
    }
    dir[2] = 1.f;
    batch.rayTest(org.data(), dir.data(), P, 5.f, dist.data());
    CHECK(dist[0] == -1.f);
    worst = 0;
    for (size_t k = 1; k < dist.size(); ++k) {
      const double ref = org[3 * k + 2] - hm.getHeight(org[3 * k], org[3 * k + 1]);
      worst = std::max(worst, std::fabs(dist[k] - ref) / (1.0 + 5.0));
    }
    std::printf("rays: max |dev - ref| / (1 + max_dist) = %.3g\n", worst);
    CHECK(worst <= 1e-5);
    std::printf("terrain_query_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
