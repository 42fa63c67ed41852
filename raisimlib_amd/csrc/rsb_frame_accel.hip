// rsb_frame_accel.hip — batched frame accelerations, frame Jacobian rates and IMU readings from the resident state
// (rsb_get_frame_accelerations, rsb_get_frame_jacobian_rates, rsb_imu_observe; include/rsb.h).
//
// The second time derivative of what rsb_frames.hip gives: what ArticulatedSystem::getFrameAcceleration / getTimeDerivativeOfSparseJacobian /
// getTimeDerivativeOfSparseRotationalJacobian give for one object on the host [RECALL], and the accelerometer + gyro rows of an observation, for all
// N envs in one call, from d_gc / d_gv on the world's stream.  Nothing here is shared with the step kernel: two short kernels of their own, called
// between two control steps, that write nothing but their outputs.  The chain walk, the argument checks and the staging of the RSB_HOST forms are
// those of the other batched queries (frames_chain.h).
//
// With (R, p, omega, v, alpha, acc) of the frame's body i from walk_chain<ACC> (acc: the classical acceleration of the body's origin) and
// o = R offset:
//     lin_acc = acc + alpha x o + omega x (omega x o) = J_lin udot + Jdot_lin gv          ang_acc = alpha = J_rot udot + Jdot_rot gv
// and, column by column, with (a_j, p_j, omega_j, v_j) of chain body j, the point (p, v) and d/dt a_j = omega_j x a_j:
//     base linear      Jdot_lin = 0                                                    Jdot_rot = 0
//     base angular k   Jdot_lin = e_k x (v - v_base)                                   Jdot_rot = 0
//     revolute j       Jdot_lin = (omega_j x a_j) x (p - p_j) + a_j x (v - v_j)        Jdot_rot = omega_j x a_j
//     prismatic j      Jdot_lin = omega_j x a_j                                        Jdot_rot = 0
// What a lane computes depends on its (env, frame) alone, so a frame's results do not depend on which other frames a call lists, or in which order.
//
//   frame_accel_kernel           one lane per (env, frame), env-major; the model rows are staged into LDS once per workgroup.  One instruction
//                                stream: udot == NULL, RSB_ACC_LOCAL, RSB_ACC_PROPER and "two [N,F,3] outputs or one IMU row" are run-time,
//                                workgroup-uniform branches.  The IMU row is the LOCAL | PROPER acceleration and R^T omega, six floats per frame at
//                                the caller's row pitch.
//   frame_jacobian_rates_kernel  the two phases of frame_jacobians_kernel: a workgroup takes `ppb` consecutive pairs - a CONTIGUOUS range of
//                                ppb * 3 * nv floats of each output; (1) one lane per pair walks the chain with velocities and leaves a head
//                                record (point, its velocity, base position, base velocity, body) and one record per level (a_j, p_j,
//                                omega_j x a_j, v_j, joint type) in LDS; (2) all lanes sweep the output range, consecutive lanes writing
//                                consecutive floats: an element is 0 unless its column is a base column or DevModel::anc puts its body on the chain.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kRateHead = 13;         // rates kernel, per pair in LDS: point 0-2, its velocity 3-5, base position 6-8, base velocity 9-11, body 12
constexpr int kRateLevel = 13;        // ... then per level >= 1: a 0-2, p 3-5, omega x a 6-8, v 9-11, joint type 12 (1 revolute, 2 prismatic)
constexpr int kRateLdsFloats = 12288; // chain records per workgroup (48 KB): bounds the pairs per workgroup for deep trees

__global__ __launch_bounds__(kThreads) void frame_accel_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                               const float* __restrict__ udot, const FrameList frames, int F, int N, const Vec3 g, int flags,
                                                               float* __restrict__ lin_acc, float* __restrict__ ang_acc, float* __restrict__ imu,
                                                               long long row_stride) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  const DevModel& m = *model;
  stage_rows(m, rows);
  __syncthreads();
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long long)N * F) return;
  const int env = (int)(idx / F), fr = (int)(idx - (long long)env * F);
  const rsb_frame f = frames.f[fr];
  const float* q = gc + (size_t)env * m.nq;
  const float* u = gv + (size_t)env * m.nv;
  const float* ud = udot ? udot + (size_t)env * m.nv : nullptr;
  Chain c;
  walk_chain<true>(m, rows, q, u, ud, true, f.body, c, NoJoint{});
  float o[3], ao[3], wo[3], wwo[3], a[3], al[3], w[3];
  mat3_vec(c.R, f.offset, o);
  cross3(c.al, o, ao);
  cross3(c.w, o, wo);
  cross3(c.w, wo, wwo);
  for (int k = 0; k < 3; ++k) { a[k] = c.ac[k] + ao[k] + wwo[k]; al[k] = c.al[k]; w[k] = c.w[k]; }
  if (flags & RSB_ACC_PROPER) { a[0] -= g.x; a[1] -= g.y; a[2] -= g.z; }
  if (flags & RSB_ACC_LOCAL) {
    float t[3];
    mat3t_vec(c.R, a, t);
    for (int k = 0; k < 3; ++k) a[k] = t[k];
    mat3t_vec(c.R, al, t);
    for (int k = 0; k < 3; ++k) al[k] = t[k];
    mat3t_vec(c.R, w, t);
    for (int k = 0; k < 3; ++k) w[k] = t[k];
  }
  if (imu) {
    float* row = imu + (long long)env * row_stride + 6 * fr;
    for (int k = 0; k < 3; ++k) { row[k] = a[k]; row[3 + k] = w[k]; }
  } else {
    if (lin_acc) for (int k = 0; k < 3; ++k) lin_acc[idx * 3 + k] = a[k];
    if (ang_acc) for (int k = 0; k < 3; ++k) ang_acc[idx * 3 + k] = al[k];
  }
}

// dynamic LDS: [nb * kRow model rows | ppb chain records of `pitch` floats]
__global__ __launch_bounds__(kThreads) void frame_jacobian_rates_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                                        const FrameList frames, int F, int N, int ppb, int pitch, float* __restrict__ Jdot_lin,
                                                                        float* __restrict__ Jdot_rot) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DevModel& m = *model;
  float* rows = lds;
  float* chains = lds + m.nb * kRow;
  stage_rows(m, rows);
  __syncthreads();
  const long long pairs = (long long)N * F, pair0 = (long long)blockIdx.x * ppb;
  const int here = (int)min((long long)ppb, pairs - pair0);
  if ((int)threadIdx.x < here) {
    const long long idx = pair0 + threadIdx.x;
    const int env = (int)(idx / F), fr = (int)(idx - (long long)env * F);
    const rsb_frame f = frames.f[fr];
    const float* q = gc + (size_t)env * m.nq;
    const float* u = gv + (size_t)env * m.nv;
    float* ch = chains + threadIdx.x * pitch;
    Chain c;
    walk_chain<false>(m, rows, q, u, nullptr, true, f.body, c, [ch, &c](int l, int, const float* a, const float* p, bool revolute) {
      float* s = ch + kRateHead + (l - 1) * kRateLevel;      // (c is the joint's own body here: its omega and v)
      float wa[3];
      cross3(c.w, a, wa);
      for (int k = 0; k < 3; ++k) { s[k] = a[k]; s[3 + k] = p[k]; s[6 + k] = wa[k]; s[9 + k] = c.v[k]; }
      s[12] = revolute ? 1.f : 2.f;
    });
    const bool moves = !m.fixed_base;
    float o[3], wo[3];
    mat3_vec(c.R, f.offset, o);
    cross3(c.w, o, wo);
    for (int k = 0; k < 3; ++k) { ch[k] = c.p[k] + o[k]; ch[3 + k] = c.v[k] + wo[k]; ch[6 + k] = q[k]; ch[9 + k] = moves ? u[k] : 0.f; }
    ch[12] = __int_as_float(f.body);
  }
  __syncthreads();
  const int nv = m.nv, per = 3 * nv, depth = m.depth;
  const bool fixed = m.fixed_base != 0;
  const size_t out0 = (size_t)pair0 * per;
  for (int e = threadIdx.x; e < here * per; e += kThreads) {
    const int k = e / per, rem = e - k * per, r = rem / nv, d = rem - r * nv;
    const float* ch = chains + k * pitch;
    const int r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;     // (r + 1) % 3, (r + 2) % 3
    float jl = 0.f, jr = 0.f;
    if (d < 6) {
      if (!fixed && d >= 3) {                                        // -[v - v_base]x
        const int c = d - 3;
        if (c == r1) jl = ch[3 + r2] - ch[9 + r2];
        else if (c == r2) jl = -(ch[3 + r1] - ch[9 + r1]);
      }
    } else {
      const int j = d - 5, lj = m.level[j];
      if (m.anc[__float_as_int(ch[12]) * depth + lj] == j) {         // body j carries the frame
        const float* s = ch + kRateHead + (lj - 1) * kRateLevel;
        if (s[12] == 1.f) {
          jl = (s[6 + r1] * (ch[r2] - s[3 + r2]) - s[6 + r2] * (ch[r1] - s[3 + r1]))          // ((omega x a) x (p - p_j))_r
             + (s[r1] * (ch[3 + r2] - s[9 + r2]) - s[r2] * (ch[3 + r1] - s[9 + r1]));         // (a x (v - v_j))_r
          jr = s[6 + r];
        } else {
          jl = s[6 + r];
        }
      }
    }
    if (Jdot_lin) Jdot_lin[out0 + e] = jl;
    if (Jdot_rot) Jdot_rot[out0 + e] = jr;
  }
}

}  // namespace

// the launch both acceleration entry points share (rsb_world.h): exactly one of (lin_acc / ang_acc) and imu is asked for
void launch_accel(rsb_world* w, const rsb_frame* frames, int n_frames, const float* udot, int flags, float* lin_acc, float* ang_acc, float* imu,
                  long long row_stride) {
  const size_t pairs = (size_t)w->N * n_frames;
  hipLaunchKernelGGL(frame_accel_kernel, dim3(blocks_for(pairs)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc,
                     (const float*)w->d_gv, udot, frame_list(frames, n_frames), n_frames, w->N, gravity_of(w), flags, lin_acc, ang_acc, imu, row_stride);
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_get_frame_accelerations(rsb_world* w, const rsb_frame* frames, int n_frames, const float* udot, int flags, float* lin_acc, float* ang_acc, int space) {
  const char* who = "rsb_get_frame_accelerations";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (flags & ~(RSB_ACC_LOCAL | RSB_ACC_PROPER)) return invalid(who, "unknown flag bits");
  if (!lin_acc && !ang_acc) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames;
  const float* dud;
  float *dl, *da;
  Staged io(w, space);
  io.in(dud, udot, (size_t)w->N * w->blob.nv); io.out(dl, lin_acc, pairs * 3); io.out(da, ang_acc, pairs * 3);
  st = io.begin(); if (st != RSB_OK) return st;
  launch_accel(w, frames, n_frames, dud, flags, dl, da, nullptr, 0);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_get_frame_jacobian_rates(rsb_world* w, const rsb_frame* frames, int n_frames, float* Jdot_lin, float* Jdot_rot, int space) {
  const char* who = "rsb_get_frame_jacobian_rates";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!Jdot_lin && !Jdot_rot) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames, per = pairs * 3 * w->blob.nv;
  float *dl, *dr;
  Staged io(w, space);
  io.out(dl, Jdot_lin, per); io.out(dr, Jdot_rot, per);
  st = io.begin(); if (st != RSB_OK) return st;
  const int pitch = (kRateHead + kRateLevel * std::max(1, w->blob.depth - 1)) | 1;      // odd: the lanes of phase 1 write to different banks
  const int ppb = std::max(1, std::min(64, kRateLdsFloats / pitch));
  const size_t lds = ((size_t)w->blob.nb * kRow + (size_t)ppb * pitch) * sizeof(float);
  hipLaunchKernelGGL(frame_jacobian_rates_kernel, dim3(blocks_for(pairs, ppb)), dim3(kThreads), lds, stream_of(w), (const DevModel*)w->d_model,
                     (const float*)w->d_gc, (const float*)w->d_gv, frame_list(frames, n_frames), n_frames, w->N, ppb, pitch, dl, dr);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_imu_observe(rsb_world* w, const rsb_frame* frames, int n_frames, const float* udot, float* out, long long row_stride, int space) {
  const char* who = "rsb_imu_observe";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!out) return invalid(who, "out must not be NULL");
  const long long width = 6LL * n_frames;
  if (row_stride == 0) row_stride = width;
  if (row_stride < width) return invalid(who, "row_stride " + std::to_string(row_stride) + " is smaller than 6 * n_frames = " + std::to_string(width));
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  const float* dud;
  float* dout;
  Staged io(w, space);      // RSB_HOST: the rows are staged dense; they go to the caller's stride on the way back, below, not through end()
  io.in(dud, udot, N * w->blob.nv); io.out(dout, out, N * width);
  st = io.begin(); if (st != RSB_OK) return st;
  hipStream_t s = stream_of(w);
  launch_accel(w, frames, n_frames, dud, RSB_ACC_LOCAL | RSB_ACC_PROPER, nullptr, nullptr, dout, space == RSB_HOST ? width : row_stride);
  HIP_TRY(hipGetLastError());
  if (space == RSB_HOST) {
    const int fs = fault_status(w); if (fs != RSB_OK) return fs;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)row_stride * sizeof(float), dout, (size_t)width * sizeof(float), (size_t)width * sizeof(float), N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return RSB_OK;
}

}  // extern "C"
