// rsb_frames.hip — batched frame kinematics, frame Jacobians and external wrenches from the resident state
// (rsb_get_frame_kinematics, rsb_get_frame_jacobians, rsb_add_external_wrench; include/rsb.h).
//
// What ArticulatedSystem::getFramePosition / getFrameOrientation / getFrameVelocity / getFrameAngularVelocity / getDenseFrameJacobian /
// getDenseFrameRotationalJacobian / setExternalForce / setExternalTorque give for one object on the host [RECALL], for all N envs in one call, from
// d_gc / d_gv / d_tff on the world's stream.  Nothing here is shared with the step kernel: these are short kernels of their own, called between two
// control steps.  What they share with the other batched queries - the chain walk, the argument checks, the staging of the RSB_HOST forms - is in
// frames_chain.h.
//
// A frame is a point fixed in a body (rsb_frame: body, offset in the body frame).  Its support chain is the path root -> body, at most `depth` bodies,
// listed by DevModel::anc.  Every kernel walks that chain with the running world transform (R, p) and velocity (omega, v) of the current body in
// REGISTERS (walk_chain, frames_chain.h): no per-body arrays, no scratch, no cross-lane traffic.
//     p_i = p_p + R_p ptree_i (+ a_i q_i, prismatic)      R_i = R_p rtree_i Rot(axis_i, q_i)      a_i = R_i axis_i
//     v_i = v_p + omega_p x (p_i - p_p) (+ a_i qd_i, prismatic)      omega_i = omega_p (+ a_i qd_i, revolute)
//     point = p_i + R_i offset      v_point = v_i + omega_i x R_i offset
// What a lane computes depends on its (env, frame) alone, so a frame's results do not depend on which other frames a call lists, or in which order.
//
//   frame_kinematics_kernel  one lane per (env, frame), env-major: the [N,F,3] / [N,F,9] stores of consecutive lanes are adjacent in memory.  The
//                            model rows (kRow floats per body) are staged into LDS once per workgroup.  A NULL output costs a uniform branch.
//   frame_jacobians_kernel   the rows of a Jacobian are 3 nv floats per (env, frame): a lane per pair would store with a stride of 3 nv floats.  A
//                            workgroup takes `ppb` consecutive pairs - a CONTIGUOUS range of ppb * 3 * nv floats of each output - in two phases:
//                            (1) one lane per pair walks the chain and leaves the point, the base position and (a_l, p_l, joint type) of every
//                            level in LDS; (2) all lanes sweep the output range, consecutive lanes writing consecutive floats: element (row r,
//                            column d) is 0 unless d is a base column or body d - 5 is on the chain (DevModel::anc says so), else one cross-product
//                            component from LDS.  (A lane per (env, frame, column) writes as well but walks the chain nv times per pair.)
//   external_wrench_kernel   one lane per env: the chain is walked twice - first for the point (the lever arms need it), then adding
//                            a_l . (torque + (point - p_l) x force) (revolute) or a_l . force (prismatic) to the <= 6 + depth entries of the env's
//                            tau_ff row the chain touches.  The row belongs to this lane: plain loads and stores, no atomics.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kChainHead = 8;        // Jacobian kernel, per pair in LDS: point 0-2, base position 3-5, body 6, -; then kChainLevel floats per level >= 1
constexpr int kChainLevel = 7;       // a 0-2, p 3-5, revolute 6
constexpr int kJacLdsFloats = 12288; // chain records per workgroup (48 KB): bounds the pairs per workgroup for deep trees

__global__ __launch_bounds__(kThreads) void frame_kinematics_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                                    const FrameList frames, int F, int N, float* __restrict__ pos, float* __restrict__ rot,
                                                                    float* __restrict__ lin_vel, float* __restrict__ ang_vel) {
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
  Chain c;
  walk_chain<false>(m, rows, q, u, nullptr, lin_vel || ang_vel, f.body, c, NoJoint{});      // (one instruction stream for the transform, whichever outputs are asked for)
  float o[3];
  mat3_vec(c.R, f.offset, o);
  if (pos) for (int k = 0; k < 3; ++k) pos[idx * 3 + k] = c.p[k] + o[k];
  if (rot) for (int k = 0; k < 9; ++k) rot[idx * 9 + k] = c.R[k];
  if (lin_vel) {
    float wo[3];
    cross3(c.w, o, wo);
    for (int k = 0; k < 3; ++k) lin_vel[idx * 3 + k] = c.v[k] + wo[k];
  }
  if (ang_vel) for (int k = 0; k < 3; ++k) ang_vel[idx * 3 + k] = c.w[k];
}

// dynamic LDS: [nb * kRow model rows | ppb chain records of `pitch` floats]
__global__ __launch_bounds__(kThreads) void frame_jacobians_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const FrameList frames, int F, int N,
                                                                   int ppb, int pitch, float* __restrict__ J_lin, float* __restrict__ J_rot) {
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
    float* ch = chains + threadIdx.x * pitch;
    Chain c;
    walk_chain<false>(m, rows, q, nullptr, nullptr, false, f.body, c, [ch](int l, int, const float* a, const float* p, bool revolute) {
      float* s = ch + kChainHead + (l - 1) * kChainLevel;
      for (int k = 0; k < 3; ++k) { s[k] = a[k]; s[3 + k] = p[k]; }
      s[6] = revolute ? 1.f : 0.f;
    });
    float o[3];
    mat3_vec(c.R, f.offset, o);
    for (int k = 0; k < 3; ++k) { ch[k] = c.p[k] + o[k]; ch[3 + k] = q[k]; }
    ch[6] = __int_as_float(f.body);
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
      if (!fixed) {
        if (d < 3) jl = d == r ? 1.f : 0.f;
        else {                                                       // -[point - p_base]x
          const int c = d - 3;
          if (c == r1) jl = ch[r2] - ch[3 + r2];
          else if (c == r2) jl = -(ch[r1] - ch[3 + r1]);
          jr = c == r ? 1.f : 0.f;
        }
      }
    } else {
      const int j = d - 5, lj = m.level[j];
      if (m.anc[__float_as_int(ch[6]) * depth + lj] == j) {          // body j carries the frame
        const float* s = ch + kChainHead + (lj - 1) * kChainLevel;
        if (s[6] != 0.f) {
          jl = s[r1] * (ch[r2] - s[3 + r2]) - s[r2] * (ch[r1] - s[3 + r1]);   // (a x (point - p_j))_r
          jr = s[r];
        } else {
          jl = s[r];
        }
      }
    }
    if (J_lin) J_lin[out0 + e] = jl;
    if (J_rot) J_rot[out0 + e] = jr;
  }
}

__global__ __launch_bounds__(kThreads) void external_wrench_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const rsb_frame f, int N,
                                                                   const float* __restrict__ force, const float* __restrict__ torque,
                                                                   const uint8_t* __restrict__ mask, float* __restrict__ tau_ff) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  const DevModel& m = *model;
  stage_rows(m, rows);
  __syncthreads();
  const int env = blockIdx.x * kThreads + threadIdx.x;
  if (env >= N || (mask && !mask[env])) return;
  const float* q = gc + (size_t)env * m.nq;
  float* tau = tau_ff + (size_t)env * m.nv;
  float fo[3], to[3], pt[3], o[3];
  for (int k = 0; k < 3; ++k) { fo[k] = force ? force[(size_t)env * 3 + k] : 0.f; to[k] = torque ? torque[(size_t)env * 3 + k] : 0.f; }
  Chain c;
  // (an empty callback of this kernel's own, not NoJoint: profiles/query_common_isa.txt says what the shared one cost when this was written; worth another look with a new compiler)
  walk_chain<false>(m, rows, q, nullptr, nullptr, false, f.body, c, [](int, int, const float*, const float*, bool) {});
  mat3_vec(c.R, f.offset, o);
  for (int k = 0; k < 3; ++k) pt[k] = c.p[k] + o[k];
  if (!m.fixed_base) {
    const float r[3] = {pt[0] - q[0], pt[1] - q[1], pt[2] - q[2]};
    float rf[3];
    cross3(r, fo, rf);
    for (int k = 0; k < 3; ++k) { tau[k] += fo[k]; tau[3 + k] += to[k] + rf[k]; }
  }
  walk_chain<false>(m, rows, q, nullptr, nullptr, false, f.body, c, [&](int, int i, const float* a, const float* p, bool revolute) {
    float g;
    if (revolute) {
      const float r[3] = {pt[0] - p[0], pt[1] - p[1], pt[2] - p[2]};
      float rf[3];
      cross3(r, fo, rf);
      for (int k = 0; k < 3; ++k) rf[k] += to[k];
      g = dot3(a, rf);
    } else {
      g = dot3(a, fo);
    }
    tau[5 + i] += g;
  });
}

}  // namespace

// the staging buffer of the batched queries' RSB_HOST forms (Staged, frames_chain.h), at least `floats` long (grown between launches: everything enqueued so far is waited for first)
int staging(rsb_world* w, size_t floats) {
  if (w->frames_io_cap >= floats) return RSB_OK;
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  if (w->d_frames_io) HIP_TRY(hipFree(w->d_frames_io));
  w->d_frames_io = nullptr; w->frames_io_cap = 0;
  HIP_TRY(hipMalloc(&w->d_frames_io, floats * sizeof(float)));
  w->frames_io_cap = floats;
  return RSB_OK;
}

void frames_free(rsb_world* w) {
  if (w->d_frames_io) (void)hipFree(w->d_frames_io);
  w->d_frames_io = nullptr; w->frames_io_cap = 0;
}

// frame_kinematics_kernel enqueued on the world's stream (rsb_world.h): device pointers, any output may be null
void launch_frame_kinematics(rsb_world* w, const rsb_frame* frames, int n_frames, float* pos, float* rot, float* lin_vel, float* ang_vel) {
  const size_t pairs = (size_t)w->N * n_frames;
  hipLaunchKernelGGL(frame_kinematics_kernel, dim3(blocks_for(pairs)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc,
                     (const float*)w->d_gv, frame_list(frames, n_frames), n_frames, w->N, pos, rot, lin_vel, ang_vel);
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_get_frame_kinematics(rsb_world* w, const rsb_frame* frames, int n_frames, float* pos, float* rot, float* lin_vel, float* ang_vel, int space) {
  const char* who = "rsb_get_frame_kinematics";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!pos && !rot && !lin_vel && !ang_vel) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames;
  float *dp, *dr, *dl, *da;
  Staged io(w, space);
  io.out(dp, pos, pairs * 3); io.out(dr, rot, pairs * 9); io.out(dl, lin_vel, pairs * 3); io.out(da, ang_vel, pairs * 3);
  st = io.begin(); if (st != RSB_OK) return st;
  launch_frame_kinematics(w, frames, n_frames, dp, dr, dl, da);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_get_frame_jacobians(rsb_world* w, const rsb_frame* frames, int n_frames, float* J_lin, float* J_rot, int space) {
  const char* who = "rsb_get_frame_jacobians";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!J_lin && !J_rot) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames, per = pairs * 3 * w->blob.nv;
  float *dl, *dr;
  Staged io(w, space);
  io.out(dl, J_lin, per); io.out(dr, J_rot, per);
  st = io.begin(); if (st != RSB_OK) return st;
  const int pitch = (kChainHead + kChainLevel * std::max(1, w->blob.depth - 1)) | 1;      // odd: the lanes of phase 1 write to different banks
  const int ppb = std::max(1, std::min(64, kJacLdsFloats / pitch));
  const size_t lds = ((size_t)w->blob.nb * kRow + (size_t)ppb * pitch) * sizeof(float);
  hipLaunchKernelGGL(frame_jacobians_kernel, dim3(blocks_for(pairs, ppb)), dim3(kThreads), lds, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc,
                     frame_list(frames, n_frames), n_frames, w->N, ppb, pitch, dl, dr);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_add_external_wrench(rsb_world* w, const rsb_frame* frame, const float* force, const float* torque, const uint8_t* mask, int space) {
  const char* who = "rsb_add_external_wrench";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frame, frame ? 1 : 0); if (st != RSB_OK) return st;
  if (!force && !torque) return invalid(who, "force and torque are both NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  const float *df, *dq;
  const uint8_t* dm;
  Staged io(w, space);      // no output: end() waits for the stream, the caller may reuse its host buffers
  io.in(df, force, 3 * N); io.in(dq, torque, 3 * N); io.in(dm, mask, N);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(external_wrench_kernel, dim3(blocks_for(N)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc, *frame, w->N,
                     df, dq, dm, w->d_tff);
  HIP_TRY(hipGetLastError());
  w->tff_zero = false;      // the step kernel reads the feed-forward rows from now on
  return io.end();
}

}  // extern "C"
