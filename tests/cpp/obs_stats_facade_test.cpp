// Compiles against include/raisim/*.hpp only and links librsb.so: DeviceVectorizedEnvironment with the running observation statistics on the
// device (VecEnvConfig::normalize_observation / obs_clip, observe(.., updateStatistics), observeDevice(.., updateStatistics), getObStatistics,
// setObStatistics, updateObStatistics, rolloutMlp with the live statistics).  Exit code 0 = all checks passed, 1 = a check failed or no device.
#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "raisim/VectorizedEnvironment.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: obs_stats_facade_test <urdf>\n"); return 2; }
  const std::string urdf = argv[1];
  try {
    const int n = 256, od = 34, ad = 12;
    raisim::VecEnvConfig cfg;
    cfg.num_envs = n;
    cfg.normalize_observation = true;
    cfg.obs_clip = 5.0;
    raisim::DeviceVectorizedEnvironment env(urdf, cfg);
    env.init();
    std::vector<float> mean(od), var(od), ob((size_t)n * od), act((size_t)n * ad), rew(n);
    std::unique_ptr<bool[]> done(new bool[n]);
    float count = 0.f;
    env.getObStatistics(mean.data(), var.data(), count);
    for (int j = 0; j < od; ++j) CHECK(mean[j] == 0.f && var[j] == 1.f);
    CHECK(count == 1e-4f);
    unsigned s = 777u;
    for (int it = 0; it < 5; ++it) {
      for (auto& a : act) { s = s * 1664525u + 1013904223u; a = ((s >> 8) / 16777216.0f - 0.5f) * 2.0f; }
      env.step(act.data(), n, ad, rew.data(), done.get());
      env.observe(ob.data(), n, od, true);
      for (float x : ob) CHECK(std::isfinite(x) && std::fabs(x) <= 5.0f);
    }
    env.getObStatistics(mean.data(), var.data(), count);
    CHECK(count == (float)(1e-4 + 5.0 * n));
    for (int j = 0; j < od; ++j) CHECK(std::isfinite(mean[j]) && var[j] >= 0.f);
    env.observe(ob.data(), n, od, false);      // no update: the count stays
    float c2 = 0.f;
    env.getObStatistics(mean.data(), var.data(), c2);
    CHECK(c2 == count);

    // set -> get round trip
    std::vector<float> m2(od), v2(od), m3(od), v3(od);
    for (int j = 0; j < od; ++j) { m2[j] = 0.1f * j - 1.f; v2[j] = 0.5f + 0.25f * j; }
    env.setObStatistics(m2.data(), v2.data(), 1234.5f);
    env.getObStatistics(m3.data(), v3.data(), c2);
    for (int j = 0; j < od; ++j) CHECK(m3[j] == m2[j] && v3[j] == v2[j]);
    CHECK(c2 == 1234.5f);

    // updateObStatistics over a device buffer of two batches: count grows by 2 n
    void* dob = nullptr;
    RSB_CHECK(rsb_device_alloc(env.world().handle(), 2 * ob.size() * sizeof(float), &dob));
    env.observeDevice(static_cast<float*>(dob));                                     // raw
    env.observeDevice(static_cast<float*>(dob) + ob.size(), false);                  // normalised, no update
    env.updateObStatistics(static_cast<const float*>(dob), 2);
    env.getObStatistics(m3.data(), v3.data(), c2);
    CHECK(c2 == (float)(1234.5 + 2.0 * n));

    // the actor network in the loop reads the live statistics
    const std::vector<int> dims = {od, 32, ad};
    std::vector<float> W0((size_t)od * 32), W1((size_t)32 * ad), b0(32, 0.f), b1(ad, 0.f);
    for (auto& x : W0) { s = s * 1664525u + 1013904223u; x = ((s >> 8) / 16777216.0f - 0.5f) * 0.3f; }
    for (auto& x : W1) { s = s * 1664525u + 1013904223u; x = ((s >> 8) / 16777216.0f - 0.5f) * 0.3f; }
    env.rolloutMlp(10, dims, {W0.data(), W1.data()}, {b0.data(), b1.data()}, RSB_ACT_TANH, 1.0f);
    CHECK(env.join() == RSB_OK);
    env.observe(ob.data(), n, od, false);
    for (float x : ob) CHECK(std::isfinite(x));
    RSB_CHECK(rsb_device_free(env.world().handle(), dob));
    std::printf("obs_stats_facade_test OK (count %.1f)\n", c2);
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 1;
  }
}
