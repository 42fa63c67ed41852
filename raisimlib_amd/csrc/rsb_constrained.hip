// rsb_constrained.hip — batched forward dynamics with frames held and the impulse that brings frames to a chosen velocity
// (rsb_constrained_forward_dynamics, rsb_frame_impulse; include/rsb.h, where the conventions are stated).
//
//   (G + rho I) lambda = target - a          x = x_f + JMinv^T lambda          rho = damping * max_i G[i][i]
// with G, JMinv of rsb_get_frame_delassus (m = kF rows) and, for the dynamics, x_f = udot_f = rsb_forward_dynamics(tau), a = J udot_f + Jdot gv
// (rsb_get_frame_accelerations); for the impulse x_f = 0, a = J gv (rsb_get_frame_kinematics' velocities).  Both are compositions on the world's
// stream, in the manner of rsb_forward_dynamics_derivatives: aba_kernel, frame_accel_kernel (frame_kinematics_kernel) and delassus_kernel through
// their launches of rsb_world.h leave udot_f, a, G and JMinv in the world's query buffer, and the one kernel of this file does the rest.
//
// held_solve_kernel.  m is uniform over the launch, so every loop has a workgroup-uniform trip count and plain barriers are safe.  An env gets a
// group of g lanes of ONE wave, no wider than it needs: g = 16 for m <= 16 (four feet, m = 12), 32 for m <= 32, 64 above, where lane l also owns row
// l + 64.  A workgroup takes epw consecutive envs, epw = min(256 / g, what fits in LDS): the launch has epw * g threads.
//   (1) lane i reads rows i (, i + 64) of the lower triangle of G - through the transpose, G[k][i] for k <= i, which has the same bits: consecutive
//       lanes read consecutive floats - into LDS, PACKED BY COLUMNS: entry (i, k), i >= k, at k m - k (k - 1) / 2 + i - k.  In the
//       factorisation and the forward substitution the lanes of a group then touch consecutive words of one column (no bank conflict) or all the
//       same word (a broadcast); the back substitution is the exception, see (3).  The diagonal goes
//       to the group's vector x, barrier, every lane takes its maximum in row order, rho, and d0_i = G[i][i] + rho.
//   (2) the root-free Cholesky G + rho I = W D^-1 W^T (L = W D^-1/2 is the Cholesky factor and D its squared diagonal: the pivots), left-looking,
//       one barrier per column j:  W[i][j] = A[i][j] - sum_{k<j} W[i][k] W[j][k] / D[k]  for the rows i >= j; the owner of row j has the pivot
//       D[j] = W[j][j], applies the rule of rsb.h - not above RSB_HELD_PIVOT_TOL d0_j, or not finite: the env's flag in LDS is set - and leaves 1 / D[j].
//   (3) x = target - a; forward substitution by columns (x_i -= W[i][k] / D[k] x_k for i > k, a barrier per k), the scaling by 1 / D, the back
//       substitution by rows of W^T (x_i -= W[k][i] / D[i] x_k for i < k, a barrier per k).  That last sweep reads ROW k of the column-packed
//       factor: lane i's word is m - i - 1 words from lane i + 1's, a stride that changes from lane to lane, so banks collide irregularly.  It is
//       m - 1 of the kernel's roughly m^2 / 2 LDS sweeps and was left as it is; its cost has not been measured on its own.
//   (4) lambda = x, or zeros with status 1; then the lanes of the group sweep the nv columns of JMinv, consecutive lanes reading and writing
//       consecutive floats: out_d = x_f[d] + sum_i JMinv[i][d] lambda_i in row order, in float.  A flagged env copies x_f's bits (zeros for the
//       impulse); a fixed base's six rows are written as zeros.
// Precision.  Everything runs in FLOAT: restated in numpy (tools/constrained_restatement.py, profiles/constrained_restatement.txt) the float
// factorisation meets both residual gates of tests/test_gpu_constrained.py with a margin of 10 x and more on every case, gives every env the status of
// its class, and ends at the forward errors of the double one - the inputs' own float32 errors (udot_f, G) set them.  `Real` below is the one place
// that says so.  No atomics, every sum in a fixed order, nothing of another env is read: the same bits for any N, any subset of outputs, host or
// device buffers.
// Static LDS 49 216 B: 12 288 floats shared by the workgroup's envs (m = 96: 4 656 + 2 x 96 per env, two envs per workgroup; m = 12: 102 per env, 16
// envs), one flag per env.  The array is as large for m = 12 as for m = 96, which caps a CU at three workgroups; at the benchmark's N = 4096 a launch is
// 256 (m = 12) or 512 (m = 24) workgroups on 256 CUs, so the cap does not bind there; what it costs at larger N has not been measured.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

using Real = float;                  // the factorisation's arithmetic
constexpr int kHeldReals = 12288;    // LDS of a workgroup, in Reals (48 KB)
constexpr int kHeldGroups = 16;      // at most 256 / 16 envs per workgroup

__host__ __device__ inline int held_group(int m) { return m <= 16 ? 16 : m <= 32 ? 32 : 64; }
__host__ __device__ inline int held_pitch(int m) { return (m * (m + 1) / 2 + 2 * m) | 1; }      // Reals per env: W packed, 1 / D, x; odd
__host__ __device__ inline int held_envs(int m) { const int a = kThreads / held_group(m), b = kHeldReals / held_pitch(m); return a < b ? a : b; }

// a: lin [N,F,3] and, with kk == 6, ang [N,F,3]: row kk f + c of the stacked vector is lin[f][c] for c < 3, ang[f][c - 3] above
__global__ __launch_bounds__(kThreads) void held_solve_kernel(int N, int m, int nv, int kk, int fixed_base, const float* __restrict__ G, const float* __restrict__ JMinv,
                                                              const float* __restrict__ xf, const float* __restrict__ lin, const float* __restrict__ ang,
                                                              const float* __restrict__ target, float damping, float* __restrict__ xout,
                                                              float* __restrict__ lambda, int32_t* __restrict__ status) {
  __shared__ Real lds[kHeldReals];
  __shared__ int flag[kHeldGroups];
  const int g = held_group(m), epw = held_envs(m), pitch = held_pitch(m);
  const int el = threadIdx.x / g, lane = threadIdx.x - el * g;
  const long long env = (long long)blockIdx.x * epw + el;
  const bool active = env < N;      // (el < epw by the launch's block size)
  Real* W = lds + el * pitch;
  Real* iD = W + m * (m + 1) / 2;
  Real* x = iD + m;
  const int F = m / kk;
  auto col = [m](int k) { return k * m - k * (k - 1) / 2 - k; };      // entry (i, k) at col(k) + i
  // ---- (1)
  if (lane == 0) flag[el] = 0;
  Real d0[2] = {0, 0};
  if (active) {
    const float* Ge = G + (size_t)env * m * m;
    for (int k = 0; k < m; ++k) {
      const int c = col(k);
      for (int i = lane; i < m; i += g)
        if (i >= k) W[c + i] = (Real)Ge[(size_t)k * m + i];
    }
    for (int i = lane; i < m; i += g) x[i] = (Real)Ge[(size_t)i * m + i];
  }
  __syncthreads();
  if (active) {
    float gmax = (float)x[0];
    for (int i = 1; i < m; ++i) gmax = fmaxf(gmax, (float)x[i]);
    const Real rho = (Real)(damping * gmax);
    for (int i = lane, r = 0; i < m; i += g, ++r) {
      d0[r] = W[col(i) + i] + rho;
      W[col(i) + i] = d0[r];
    }
  }
  __syncthreads();      // (x is written again below)
  // ---- (2)
  for (int j = 0; j < m; ++j) {
    if (active) {
      for (int i = lane, r = 0; i < m; i += g, ++r) {
        if (i < j) continue;
        Real s = W[col(j) + i];
        for (int k = 0; k < j; ++k) s -= W[col(k) + i] * W[col(k) + j] * iD[k];
        W[col(j) + i] = s;
        if (i == j) {
          const bool bad = !(s > (Real)RSB_HELD_PIVOT_TOL * d0[r]) || !isfinite(s);
          if (bad) flag[el] = 1;
          iD[j] = bad ? (Real)0 : (Real)1 / s;
        }
      }
    }
    __syncthreads();
  }
  // ---- (3)
  if (active) {
    for (int i = lane; i < m; i += g) {
      const int f = i / kk, c = i - f * kk;
      const size_t at = ((size_t)env * F + f) * 3;
      const float a = c < 3 ? lin[at + c] : ang[at + c - 3];
      x[i] = (Real)((target ? target[(size_t)env * m + i] : 0.f) - a);
    }
  }
  __syncthreads();
  for (int k = 0; k < m - 1; ++k) {
    if (active) {
      const Real yk = x[k] * iD[k];
      for (int i = lane; i < m; i += g)
        if (i > k) x[i] -= W[col(k) + i] * yk;
    }
    __syncthreads();
  }
  if (active)
    for (int i = lane; i < m; i += g) x[i] *= iD[i];
  __syncthreads();
  for (int k = m - 1; k >= 1; --k) {
    if (active) {
      const Real xk = x[k];
      for (int i = lane; i < m; i += g)
        if (i < k) x[i] -= W[col(i) + k] * iD[i] * xk;
    }
    __syncthreads();
  }
  // ---- (4)
  if (!active) return;
  const bool bad = flag[el] != 0;
  if (lambda)
    for (int i = lane; i < m; i += g) lambda[(size_t)env * m + i] = bad ? 0.f : (float)x[i];
  if (status && lane == 0) status[env] = bad ? RSB_HELD_SINGULAR : RSB_HELD_SOLVED;
  if (xout) {
    const float* JM = JMinv + (size_t)env * m * nv;
    for (int d = lane; d < nv; d += g) {
      float acc = xf ? xf[(size_t)env * nv + d] : 0.f;
      if (!bad)
        for (int i = 0; i < m; ++i) acc += JM[(size_t)i * nv + d] * (float)x[i];
      xout[(size_t)env * nv + d] = (fixed_base && d < 6) ? 0.f : acc;
    }
  }
}

// what both entry points check alike
int check_held(rsb_world* w, const char* who, const rsb_frame* frames, int n_frames, int flags, float damping, bool any_output, int space) {
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!any_output) return invalid(who, "every output is NULL");
  if (!frames || n_frames < 1 || n_frames > RSB_MAX_DELASSUS_FRAMES) return invalid(who, "n_frames must be 1.." + std::to_string(RSB_MAX_DELASSUS_FRAMES));
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (flags & ~RSB_DELASSUS_ANGULAR) return invalid(who, "unknown flag bits");
  if (!std::isfinite(damping) || damping < 0.f) return invalid(who, "damping must be finite and not negative");
  return RSB_OK;
}

// tau == nullptr && !dynamics: the impulse.  Every pointer but joint_diag and frames is in `space`.
int held_query(rsb_world* w, bool dynamics, const float* tau, const rsb_frame* frames, int n_frames, int flags, const float* target, const float* joint_diag,
               float damping, float* xout, float* lambda, int32_t* status, int space) {
  HIP_TRY(hipSetDevice(w->device));
  const int kk = (flags & RSB_DELASSUS_ANGULAR) ? 6 : 3, m = kk * n_frames, nv = w->blob.nv;
  const size_t N = (size_t)w->N, pairs3 = N * (size_t)n_frames * 3;
  const float *dtau, *dtarget;
  float *dx, *dl, *dst, *work;
  Staged io(w, space);      // [udot_f | lin | ang | G | JMinv | tau | target | outputs]
  io.in(dtau, tau, N * nv); io.in(dtarget, target, N * m);
  io.out(dx, xout, N * nv); io.out(dl, lambda, N * m); io.out(dst, reinterpret_cast<float*>(status), N);
  io.scratch(work, N * nv + 2 * pairs3 + N * m * m + N * m * nv);
  int st = io.begin(); if (st != RSB_OK) return st;
  hipStream_t s = stream_of(w);
  float *uf = work, *lin = uf + N * nv, *ang = lin + pairs3, *G = ang + pairs3, *JM = G + N * m * m;
  if (kk == 3) ang = nullptr;
  if (dynamics) {
    st = launch_forward_dynamics(w, s, dtau, nullptr, 0, nullptr, nullptr, 0, uf); if (st != RSB_OK) return st;
    launch_accel(w, frames, n_frames, uf, 0, lin, ang, nullptr, 0);
  } else {
    launch_frame_kinematics(w, frames, n_frames, nullptr, nullptr, lin, ang);
  }
  HIP_TRY(hipGetLastError());
  st = launch_frame_delassus(w, s, frames, n_frames, flags, joint_diag, G, JM); if (st != RSB_OK) return st;
  const int epw = held_envs(m);
  hipLaunchKernelGGL(held_solve_kernel, dim3(blocks_for(N, epw)), dim3(epw * held_group(m)), 0, s, w->N, m, nv, kk, (int)w->blob.fixed_base, (const float*)G,
                     (const float*)JM, dynamics ? (const float*)uf : nullptr, (const float*)lin, (const float*)ang, dtarget, damping, dx, dl,
                     reinterpret_cast<int32_t*>(dst));
  HIP_TRY(hipGetLastError());
  return io.end();
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_constrained_forward_dynamics(rsb_world* w, const float* tau, const rsb_frame* frames, int n_frames, int flags, const float* target_acc, float damping, float* udot,
                                     float* lambda, int32_t* status, int space) {
  const char* who = "rsb_constrained_forward_dynamics";
  const int st = check_held(w, who, frames, n_frames, flags, damping, udot || lambda || status, space); if (st != RSB_OK) return st;
  return held_query(w, true, tau, frames, n_frames, flags, target_acc, nullptr, damping, udot, lambda, status, space);
}

int rsb_frame_impulse(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, const float* target_vel, const float* joint_diag, float damping, float* dgv,
                      float* lambda, int32_t* status, int space) {
  const char* who = "rsb_frame_impulse";
  int st = check_held(w, who, frames, n_frames, flags, damping, dgv || lambda || status, space); if (st != RSB_OK) return st;
  st = check_joint_diag(w, who, joint_diag); if (st != RSB_OK) return st;
  return held_query(w, false, nullptr, frames, n_frames, flags, target_vel, joint_diag, damping, dgv, lambda, status, space);
}

}  // extern "C"
