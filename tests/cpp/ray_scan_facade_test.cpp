// Compiles against include/raisim/*.hpp only and links librsb.so: BatchedWorld::rayCast / rayScan / depthCameraRays (all envs in one call,
// computed on the device) on the ANYmal-like model standing over a ground plane, base upright (identity orientation) at a known place:
//   rayCast without bodies is rayTest bit for bit; far from the robot it gives the plane's closed form with or without bodies;
//   the camera pattern on the base frame: rayScan with RSB_RAY_OWN_BODY equals rayCast from the base's position along the same directions (the
//   base's axes are the world's) within 1e-5 (1 + max(|origin|, max_dist)); without it the base's own spheres are seen through, which can only
//   lengthen a ray; some rays stop at the robot's legs and all of those are shorter than the plane's answer;
//   RSB_RAY_PLANAR is the range times the direction's x component, RSB_RAY_MISS_MAX turns -1 into maxDist; row strides leave the other columns alone.
// Exit code 0 = all checks passed, 1 = a check failed or no device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/World.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: ray_scan_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int N = 4, W = 16, H = 12, P = W * H;
    const float maxDist = 4.f, groundZ = 0.05f;
    raisim::BatchedWorld batch(urdf, N);
    batch.addGround(groundZ);
    const int nq = batch.gcDim(), nv = batch.dof();
    CHECK(nq == 19);
    const float joints[12] = {0.03f, 0.4f, -0.8f, -0.03f, 0.4f, -0.8f, 0.03f, -0.4f, 0.8f, -0.03f, -0.4f, 0.8f};
    std::vector<float> gc((size_t)N * nq, 0.f), gv((size_t)N * nv, 0.f);
    for (int e = 0; e < N; ++e) {
      float* q = gc.data() + (size_t)e * nq;
      q[0] = 0.5f * e; q[1] = -0.25f * e; q[2] = 0.6f + 0.05f * e; q[3] = 1.f;
      std::copy(joints, joints + 12, q + 7);
    }
    batch.setState(gc.data(), gv.data());

    // the pattern: a pinhole camera looking along x, pitched down by 0.6 rad about y (rotated here, once: a frame has no orientation of its own)
    std::vector<float> dirs = raisim::BatchedWorld::depthCameraRays(W, H, 1.5);
    CHECK((int)dirs.size() == 3 * P);
    CHECK(dirs[1] > 0.f && dirs[2] > 0.f && dirs[3 * (P - 1) + 1] < 0.f && dirs[3 * (P - 1) + 2] < 0.f);      // pixel 0 is top left: y left, z up
    const double cp = std::cos(0.6), sp = std::sin(0.6);
    for (int k = 0; k < P; ++k) {
      const double x = dirs[3 * k], z = dirs[3 * k + 2];
      dirs[3 * k] = (float)(cp * x + sp * z); dirs[3 * k + 2] = (float)(-sp * x + cp * z);
    }
    const std::vector<rsb_frame> base{rsb_frame{0, {0.f, 0.f, 0.f}}};
    std::vector<float> scan((size_t)N * P), plain((size_t)N * P), own((size_t)N * P);
    std::vector<int32_t> hit((size_t)N * P), hitOwn((size_t)N * P), hitCast((size_t)N * P);
    batch.rayScan(base, dirs.data(), P, maxDist, scan.data(), 0, RSB_RAY_BODIES, hit.data());
    batch.rayScan(base, dirs.data(), P, maxDist, plain.data(), 0, 0);
    batch.rayScan(base, dirs.data(), P, maxDist, own.data(), 0, RSB_RAY_BODIES | RSB_RAY_OWN_BODY, hitOwn.data());

    // the same rays in world space
    std::vector<float> org((size_t)N * P * 3), dir((size_t)N * P * 3), cast((size_t)N * P), test((size_t)N * P), noBodies((size_t)N * P);
    for (int e = 0; e < N; ++e)
      for (int k = 0; k < P; ++k)
        for (int c = 0; c < 3; ++c) { org[((size_t)e * P + k) * 3 + c] = gc[(size_t)e * nq + c]; dir[((size_t)e * P + k) * 3 + c] = dirs[3 * k + c]; }
    batch.rayCast(org.data(), dir.data(), P, maxDist, cast.data(), hitCast.data());
    batch.rayCast(org.data(), dir.data(), P, maxDist, noBodies.data(), nullptr, false);
    batch.rayTest(org.data(), dir.data(), P, maxDist, test.data());
    int bodyHits = 0, terrainHits = 0;
    double worst = 0;
    for (size_t k = 0; k < scan.size(); ++k) {
      CHECK(noBodies[k] == test[k]);
      const double tol = 1e-5 * (1.0 + std::max({std::fabs((double)org[3 * k]), std::fabs((double)org[3 * k + 1]), std::fabs((double)org[3 * k + 2]), (double)maxDist}));
      CHECK(hitOwn[k] == hitCast[k]);      // (a world-space ray has no mount to see through: the scan with RSB_RAY_OWN_BODY is its equal)
      worst = std::max(worst, std::fabs((double)own[k] - cast[k]) / tol);
      CHECK(std::fabs((double)plain[k] - test[k]) <= tol);
      if (hit[k] >= 0) { ++bodyHits; CHECK(scan[k] >= 0.f && (test[k] < 0.f || scan[k] <= test[k])); }
      else if (hit[k] == RSB_RAY_HIT_TERRAIN) { ++terrainHits; CHECK(std::fabs((double)scan[k] - test[k]) <= tol); }
      else CHECK(hit[k] == RSB_RAY_HIT_NONE && scan[k] == -1.f && test[k] == -1.f);
      CHECK(own[k] >= 0.f ? (scan[k] < 0.f || own[k] <= scan[k] + tol) : scan[k] < 0.f);
    }
    std::printf("rayScan (own body) vs rayCast: max |scan - cast| = %.3g tol; %d rays stop at the robot, %d at the ground, of %d\n", worst, bodyHits, terrainHits, N * P);
    CHECK(worst <= 1.0 && bodyHits >= N && terrainHits >= N * P / 4);

    // the plane in closed form, far from the robot
    for (size_t k = 0; k < (size_t)N * P; ++k) {
      org[3 * k] = 20.f + 0.01f * (float)k; org[3 * k + 1] = -15.f; org[3 * k + 2] = 1.5f;
      dir[3 * k] = 0.3f; dir[3 * k + 1] = 0.f; dir[3 * k + 2] = -0.4f;
    }
    batch.rayCast(org.data(), dir.data(), P, maxDist, cast.data(), hitCast.data());
    for (size_t k = 0; k < cast.size(); ++k) { CHECK(std::fabs(cast[k] - (1.5 - groundZ) / 0.8) <= 1e-5 * (1.0 + org[3 * k])); CHECK(hitCast[k] == RSB_RAY_HIT_TERRAIN); }

    // a depth image into the tail columns of wider rows, misses as maxDist
    const int head = 3;
    std::vector<float> rows((size_t)N * (head + P), 7.f);
    batch.rayScan(base, dirs.data(), P, maxDist, rows.data() + head, head + P, RSB_RAY_BODIES | RSB_RAY_PLANAR | RSB_RAY_MISS_MAX);
    for (int e = 0; e < N; ++e) {
      for (int c = 0; c < head; ++c) CHECK(rows[(size_t)e * (head + P) + c] == 7.f);
      for (int k = 0; k < P; ++k) {
        const float range = scan[(size_t)e * P + k] < 0.f ? maxDist : scan[(size_t)e * P + k];
        CHECK(std::fabs(rows[(size_t)e * (head + P) + head + k] - (double)range * dirs[3 * k]) <= 1e-5 * (1.0 + maxDist));
      }
    }
    std::printf("ray_scan_facade_test OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
