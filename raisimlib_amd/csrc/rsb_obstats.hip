// rsb_obstats.hip — running observation statistics of the device-resident env (rsb_env_observe_normalized, rsb_env_obs_stats_*; include/rsb.h).
//
// Semantics: the template path's updateObservationStatisticsAndNormalize (include/raisim/VectorizedEnvironment.hpp), i.e. upstream
// raisimGymTorch's VectorizedEnvironment [RECALL]: count starts at 1e-4, mean at 0, var at 1; a batch of N observations (one per env) has the
// per-feature mean and POPULATION variance over the N envs and is merged as
//     tot = count + N,  mean' = mean * (count / tot) + bmean * (N / tot),
//     var' = (var * count + bvar * N + (mean - bmean)^2 * (count * N / tot)) / tot,  count' = tot;
// an observation is normalised as (ob - mean) / sqrt(var + 1e-8).
//
// Arithmetic: fp64 throughout the statistics, as the template path sums in double; the data is 0.56 MB per batch at 4096 x 34, so the
// kernels are bound by launches and memory latency, never by the fp64 rate.  Everything is enqueued on the world's stream; a fold is three
// kernels, none with atomics, each summing in a fixed order - the same input gives the same bits on every run:
//   obs_moments_kernel   grid (env blocks of kRows envs, batches): each workgroup sums its FIXED env range of one batch in one pass,
//                        s1 = sum (x - x0), s2 = sum (x - x0)^2 per feature, x0 = the batch's first row.  x - x0 of two floats of like
//                        magnitude is exact in double and so is its square, so the only rounding is in the sums, and M2 = s2 - s1^2 / n below loses nothing
//                        worth naming unless x0 lies many standard deviations from the batch mean.  Partials (s1, s2) per (batch, block, feature).
//   obs_batch_kernel     grid (batches): the block partials of a batch added in block order -> the batch's mean and population variance.
//   obs_merge_kernel     one workgroup, a thread per feature: the batches merged into the running (mean, var, count) in order, then the
//                        float views (mean, 1 / sqrt(var + eps)) the normaliser and the MLP stage read are refreshed.  The running state
//                        passes through the same loop body whether the batches come in one call or in many, and a batch's moments depend
//                        on that batch alone, so folding B batches at once gives the bits of B one-batch updates by construction.
//   obs_normalize_kernel out = clamp((in - mean) * inv_std, +-clip) over any number of rows, in place or not: the same two float operations
//                        as the MLP stage's input (stage_bodies.h), so a normalised observation is the stage's input bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "rsb_world.h"

#pragma clang fp contract(off)      // the statistics are an fp64 restatement of the template path: no fused multiply-adds that a reader cannot see

namespace rsbw {
namespace {

constexpr int kThreads = 256;        // workgroup size of every kernel here; also the largest observation size handled (obDim <= 136 for any model)
constexpr int kRows = 256;           // envs per workgroup of the moments kernel (fixed: the partials do not depend on how many batches a call holds)
constexpr int kUnroll = 8;           // loads in flight per thread in the moments kernel, batches per round of the merge
constexpr double kEps = 1e-8;
constexpr size_t kPartialBudget = 4u << 20;   // bytes of partials per chunk of batches

// Threads (s, j) = (t / D, t % D), S = kThreads / D row slices: thread (s, j) visits rows s, s + S, ... of feature j (consecutive threads read
// consecutive floats); the S slice sums are then added in slice order.
__global__ __launch_bounds__(kThreads) void obs_moments_kernel(const float* __restrict__ obs, long long batch_stride, int N, int D,
                                                               double* __restrict__ part) {
  __shared__ double red1[kThreads], red2[kThreads];
  const int blk = blockIdx.x, nblk = gridDim.x, b = blockIdx.y, nb = gridDim.y;
  const int r0 = blk * kRows, nr = min(kRows, N - r0);
  const int S = kThreads / D, t = threadIdx.x, j = t % D, s = t / D;
  const float* batch = obs + (size_t)b * (size_t)batch_stride;
  const float* base = batch + (size_t)r0 * D;
  double s1 = 0.0, s2 = 0.0;
  if (s < S) {
    const double x0 = (double)batch[j];
    int r = s;
    for (; r + (kUnroll - 1) * S < nr; r += kUnroll * S) {
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = base[(size_t)(r + u * S) * D + j];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) { const double d = (double)v[u] - x0; s1 += d; s2 += d * d; }
    }
    for (; r < nr; r += S) { const double d = (double)base[(size_t)r * D + j] - x0; s1 += d; s2 += d * d; }
  }
  red1[t] = s1; red2[t] = s2;
  __syncthreads();
  if (t < D) {
    double a1 = 0.0, a2 = 0.0;
    for (int q = 0; q < S; ++q) { a1 += red1[q * D + t]; a2 += red2[q * D + t]; }
    const size_t o = ((size_t)b * nblk + blk) * D + t;
    part[o] = a1;                                // part = [s1: nb x nblk x D | s2: nb x nblk x D]
    part[(size_t)nb * nblk * D + o] = a2;
  }
}

// batch blockIdx.x: its block partials added in block order (slices of blocks as above) -> bstat[b] = [mean D | population variance D]
__global__ __launch_bounds__(kThreads) void obs_batch_kernel(const float* __restrict__ obs, long long batch_stride, int N, int D, int nblk,
                                                             const double* __restrict__ part, double* __restrict__ bstat) {
  __shared__ double red1[kThreads], red2[kThreads];
  const int b = blockIdx.x, nb = gridDim.x;
  const int S = kThreads / D, t = threadIdx.x, j = t % D, s = t / D;
  const double* p1 = part + (size_t)b * nblk * D + j;
  const double* p2 = p1 + (size_t)nb * nblk * D;
  double a1 = 0.0, a2 = 0.0;
  if (s < S)
    for (int k = s; k < nblk; k += S) { a1 += p1[(size_t)k * D]; a2 += p2[(size_t)k * D]; }
  red1[t] = a1; red2[t] = a2;
  __syncthreads();
  if (t < D) {
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < S; ++q) { s1 += red1[q * D + t]; s2 += red2[q * D + t]; }
    const double n = (double)N, x0 = (double)obs[(size_t)b * (size_t)batch_stride + t];
    const double m2 = s2 - s1 * (s1 / n);
    bstat[(size_t)b * 2 * D + t] = x0 + s1 / n;
    bstat[(size_t)b * 2 * D + D + t] = (m2 > 0.0 ? m2 : 0.0) / n;
  }
}

// stats = [mean D | var D | count] (fp64), view = [mean D | inv_std D] (fp32).  n_batches = 0: only the views are refreshed (rsb_env_set_obs_stats).
__global__ __launch_bounds__(kThreads) void obs_merge_kernel(const double* __restrict__ bstat, int n_batches, int N, int D,
                                                             double* __restrict__ stats, float* __restrict__ view) {
  const int j = threadIdx.x;
  double count = stats[2 * D];
  __syncthreads();      // every thread has read the count before thread 0 may overwrite it
  if (j >= D) return;
  double mean = stats[j], var = stats[D + j];
  const double n = (double)N;
  for (int b0 = 0; b0 < n_batches; b0 += kUnroll) {      // (the loads of kUnroll batches first: they do not depend on the running state)
    double bm[kUnroll], bv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (b0 + u < n_batches) { bm[u] = bstat[(size_t)(b0 + u) * 2 * D + j]; bv[u] = bstat[(size_t)(b0 + u) * 2 * D + D + j]; }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (b0 + u < n_batches) {      // the template path's merge (upstream's arithmetic, in fp64)
        const double tot = count + n, d = mean - bm[u];
        mean = mean * (count / tot) + bm[u] * (n / tot);
        var = (var * count + bv[u] * n + d * d * (count * n / tot)) / tot;
        count = tot;
      }
  }
  stats[j] = mean;
  stats[D + j] = var;
  if (j == 0) stats[2 * D] = count;
  view[j] = (float)mean;
  view[D + j] = (float)(1.0 / sqrt(var + kEps));
}

// out[r, j] = clamp((in[r, j] - mean[j]) * inv_std[j], +-clip) (clip <= 0: none); threads (s, j) as in the moments kernel, grid-stride over rows
__global__ __launch_bounds__(kThreads) void obs_normalize_kernel(const float* in, float* out, long long rows, int D, const float* __restrict__ view, float clip) {
  const int S = kThreads / D, t = threadIdx.x, j = t % D, s = t / D;
  if (s >= S) return;
  const float m = view[j], is = view[D + j];
  for (long long r = (long long)blockIdx.x * S + s; r < rows; r += (long long)gridDim.x * S) {
    const size_t i = (size_t)r * D + j;
    float v = in[i];
    v -= m;
    v *= is;
    if (clip > 0.f) v = fminf(fmaxf(v, -clip), clip);
    out[i] = v;
  }
}

int ob_dim(const rsb_world* w) { return 10 + 2 * (w->blob.nv - 6); }
int env_blocks(const rsb_world* w) { return (w->N + kRows - 1) / kRows; }

int check(rsb_world* w, const char* who) {
  if (!w) return RSB_E_INVALID;
  if (!w->env_ready || !w->d_obs_stats) { rsb::set_error(std::string(who) + ": call rsb_env_configure first"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  return RSB_OK;
}

// folds n_batches batches of [N, D] (device memory, batch_stride floats apart) into the statistics, in order, on the world's stream
int fold(rsb_world* w, const float* obs, int n_batches, long long batch_stride) {
  const int D = ob_dim(w), nblk = env_blocks(w);
  const size_t per_batch = ((size_t)nblk * D * 2 + 2 * (size_t)D) * sizeof(double);     // partials (s1, s2) + the batch's (mean, var)
  if (!w->d_obs_part) {
    w->obs_part_batches = (int)std::max<size_t>(1, std::min<size_t>(1024, kPartialBudget / per_batch));
    HIP_TRY(hipMalloc(&w->d_obs_part, per_batch * w->obs_part_batches));
  }
  double* part = w->d_obs_part;
  double* bstat = part + (size_t)w->obs_part_batches * nblk * D * 2;
  hipStream_t s = stream_of(w);
  for (int b0 = 0; b0 < n_batches; b0 += w->obs_part_batches) {
    const int nb = std::min(w->obs_part_batches, n_batches - b0);
    const float* o = obs + (size_t)b0 * (size_t)batch_stride;
    hipLaunchKernelGGL(obs_moments_kernel, dim3(nblk, nb), dim3(kThreads), 0, s, o, batch_stride, w->N, D, part);
    hipLaunchKernelGGL(obs_batch_kernel, dim3(nb), dim3(kThreads), 0, s, o, batch_stride, w->N, D, nblk, (const double*)part, bstat);
    hipLaunchKernelGGL(obs_merge_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)bstat, nb, w->N, D, w->d_obs_stats, w->d_obs_view);
    HIP_TRY(hipGetLastError());
  }
  return RSB_OK;
}

int normalize(rsb_world* w, const float* in, float* out, long long rows, float clip) {
  const int D = ob_dim(w), S = kThreads / D;
  const long long blocks = std::min<long long>((rows + S - 1) / S, 4096);
  if (blocks < 1) return RSB_OK;
  hipLaunchKernelGGL(obs_normalize_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream_of(w), in, out, rows, D, (const float*)w->d_obs_view, clip);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

// uploads [mean | var | count] (host, fp64) and refreshes the views from them with the merge kernel's own arithmetic
int upload(rsb_world* w, const std::vector<double>& st) {
  hipStream_t s = stream_of(w);
  HIP_TRY(hipMemcpyAsync(w->d_obs_stats, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(obs_merge_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)nullptr, 0, w->N, ob_dim(w), w->d_obs_stats, w->d_obs_view);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));      // (st is the caller's stack)
  return RSB_OK;
}

}  // namespace

// rsb_env_configure: the statistics live as long as the world; the observation size is fixed by the model, so they start once, at the first call
int obs_stats_init(rsb_world* w) {
  if (w->d_obs_stats) return RSB_OK;
  const int D = ob_dim(w);
  if (D > kThreads) { rsb::set_error("rsb_env_configure: observation statistics support at most 256 observation entries"); return RSB_E_UNSUPPORTED; }
  HIP_TRY(hipMalloc(&w->d_obs_stats, (2 * (size_t)D + 1) * sizeof(double)));
  HIP_TRY(hipMalloc(&w->d_obs_view, 2 * (size_t)D * sizeof(float)));
  std::vector<double> st(2 * (size_t)D + 1, 0.0);
  for (int j = 0; j < D; ++j) st[D + j] = 1.0;
  st[2 * D] = 1e-4;
  return upload(w, st);
}

void obs_stats_free(rsb_world* w) {
  for (void* p : {(void*)w->d_obs_stats, (void*)w->d_obs_view, (void*)w->d_obs_part}) if (p) (void)hipFree(p);
  w->d_obs_stats = w->d_obs_part = nullptr; w->d_obs_view = nullptr;
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_env_observe_normalized(rsb_world* w, float* ob, int update_statistics, float clip, int space) {
  int st = check(w, "rsb_env_observe_normalized"); if (st != RSB_OK) return st;
  if (!ob || (space != RSB_HOST && space != RSB_DEVICE)) { rsb::set_error("rsb_env_observe_normalized: bad argument"); return RSB_E_INVALID; }
  float* dob = space == RSB_DEVICE ? ob : w->d_env_io;
  st = launch_env_obs(w, dob, stream_of(w)); if (st != RSB_OK) return st;
  if (update_statistics) { st = fold(w, dob, 1, 0); if (st != RSB_OK) return st; }
  st = normalize(w, dob, dob, w->N, clip); if (st != RSB_OK) return st;
  if (space == RSB_HOST) return copy_out(w, ob, dob, (size_t)w->N * ob_dim(w) * sizeof(float), RSB_HOST);
  return RSB_OK;
}

int rsb_env_obs_stats_update(rsb_world* w, const float* obs, int n_batches, long long batch_stride, int space) {
  int st = check(w, "rsb_env_obs_stats_update"); if (st != RSB_OK) return st;
  const long long nd = (long long)w->N * ob_dim(w);
  if (batch_stride == 0) batch_stride = nd;
  if (!obs || n_batches < 0 || batch_stride < nd || (space != RSB_HOST && space != RSB_DEVICE)) {
    rsb::set_error("rsb_env_obs_stats_update: bad argument (batches of [N, ob_dim] floats, batch_stride >= N * ob_dim or 0)");
    return RSB_E_INVALID;
  }
  if (space == RSB_DEVICE) return fold(w, obs, n_batches, batch_stride);
  for (int b = 0; b < n_batches; ++b) {      // host batches through the staging buffer, one at a time (the same bits: see the top of this file)
    HIP_TRY(hipMemcpyAsync(w->d_env_io, obs + (size_t)b * (size_t)batch_stride, (size_t)nd * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    st = fold(w, w->d_env_io, 1, nd); if (st != RSB_OK) return st;
  }
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  return RSB_OK;
}

int rsb_env_obs_normalize(rsb_world* w, const float* in, float* out, long long rows, float clip, int space) {
  int st = check(w, "rsb_env_obs_normalize"); if (st != RSB_OK) return st;
  if (!in || !out || rows < 0 || (space != RSB_HOST && space != RSB_DEVICE)) { rsb::set_error("rsb_env_obs_normalize: bad argument"); return RSB_E_INVALID; }
  if (space == RSB_DEVICE) return normalize(w, in, out, rows, clip);
  const int D = ob_dim(w);
  for (long long r0 = 0; r0 < rows; r0 += w->N) {      // host rows through the staging buffer [N, D], N rows at a time
    const long long nr = std::min<long long>(w->N, rows - r0);
    const size_t bytes = (size_t)nr * D * sizeof(float);
    HIP_TRY(hipMemcpyAsync(w->d_env_io, in + (size_t)r0 * D, bytes, hipMemcpyHostToDevice, stream_of(w)));
    st = normalize(w, w->d_env_io, w->d_env_io, nr, clip); if (st != RSB_OK) return st;
    st = copy_out(w, out + (size_t)r0 * D, w->d_env_io, bytes, RSB_HOST); if (st != RSB_OK) return st;
  }
  return RSB_OK;
}

int rsb_env_get_obs_stats(rsb_world* w, float* mean, float* var, double* count) {
  int st = check(w, "rsb_env_get_obs_stats"); if (st != RSB_OK) return st;
  const int D = ob_dim(w);
  std::vector<double> h(2 * (size_t)D + 1);
  st = copy_out(w, h.data(), w->d_obs_stats, h.size() * sizeof(double), RSB_HOST); if (st != RSB_OK) return st;
  for (int j = 0; j < D; ++j) {
    if (mean) mean[j] = (float)h[j];
    if (var) var[j] = (float)h[D + j];
  }
  if (count) *count = h[2 * D];
  return RSB_OK;
}

int rsb_env_set_obs_stats(rsb_world* w, const float* mean, const float* var, double count) {
  int st = check(w, "rsb_env_set_obs_stats"); if (st != RSB_OK) return st;
  if (!mean || !var || !(count >= 0.0)) { rsb::set_error("rsb_env_set_obs_stats: bad argument (mean and var [ob_dim], count >= 0)"); return RSB_E_INVALID; }
  const int D = ob_dim(w);
  std::vector<double> h(2 * (size_t)D + 1);
  for (int j = 0; j < D; ++j) { h[j] = mean[j]; h[D + j] = var[j]; }
  h[2 * D] = count;
  return upload(w, h);
}

int rsb_env_obs_stats_device(rsb_world* w, const float** mean, const float** inv_std) {
  int st = check(w, "rsb_env_obs_stats_device"); if (st != RSB_OK) return st;
  if (mean) *mean = w->d_obs_view;
  if (inv_std) *inv_std = w->d_obs_view + ob_dim(w);
  return RSB_OK;
}

}  // extern "C"
