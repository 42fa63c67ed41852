// rsb_contact_sensor.hip — batched contact sensors from the resident contact list: the net contact wrench on a body, the contact rows of an
// observation (contact flag, net force, normal force, slip speed) and feet air time / contact time
// (rsb_get_body_contact_wrenches, rsb_contact_observe, rsb_contact_timers; include/rsb.h).
//
// What a caller of ArticulatedSystem::getContacts() loops over on the host for one object [RECALL], reduced per (env, frame) for all N envs in one
// call, from d_contacts / d_count / d_gc / d_gv on the world's stream.  Nothing here is shared with the step kernel: one kernel of its own, called
// between two control steps, that writes nothing but its outputs.  The chain walk, the argument checks and the staging of the RSB_HOST forms are
// those of the other batched queries (frames_chain.h).
//
// A record c < min(count[e], kmax) of env e acts as the world force f_c = impulse_c * inv_dt at position_c on body_c, inv_dt = (float)(1 / dt): the
// convention of RSB_DYN_CONTACTS (rsb_dynamics.hip).  A frame owns the records of its body.  With (R, p_b, omega_b, v_b) of the frame's body from
// walk_chain and p_f = p_b + R offset:
//     force  = sum f_c                                  torque = sum (position_c - p_f) x f_c
//     normal = sum (impulse_c . normal_c) * inv_dt      slip   = max |v - (v . n_c) n_c|,  v = v_b + omega_b x (position_c - p_b)
// The torque's lever is taken from the frame's point, never from the world origin: an env standing 50 m away loses the bits of position_c alone.
//
//   contact_sensor_kernel   a workgroup takes epb = min(256 / F, what fits in LDS) CONSECUTIVE envs and one lane per (env, frame), env-major.  The
//                           model rows, the envs' counts and their records - a contiguous range of 12-dword records - are staged into LDS first,
//                           consecutive lanes loading consecutive dwords; an env's records sit at an odd pitch, so the lanes of different envs
//                           read different banks and the lanes of one env read one address.  Each lane walks its chain once (with velocities
//                           only where slip is asked for), then loops over its env's records in ascending index and accumulates in registers: no
//                           atomics, a fixed order.  One instruction stream: the flags, NULL outputs and "separate outputs, six-float row or
//                           timers" are run-time, workgroup-uniform branches, so `force` carries the same bits from all three entry points.  The
//                           timers are the tail of the same stream: one elementwise update per lane from its own contact flag.
// A lane's result depends on its (env, frame) alone: the same bits for any N, any other frames of the call, any subset of outputs, host or device.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kRec = sizeof(rsb_contact) / 4;      // dwords of a record: position 0-2, normal 3-5, impulse 6-8, depth 9, body 10, collision 11
constexpr int kRecLdsDwords = 12288;               // counts and records per workgroup (48 KB): bounds the envs per workgroup
static_assert(kRec == 12, "rsb_contact is twelve dwords");

enum SensorMode { kWrench = 0, kObserve = 1, kTimers = 2 };

// what one launch writes.  kWrench: force / torque / count [N,F,*] (any may be null); kObserve: six floats per frame at row + e * row_stride + 6 f;
// kTimers: air / ct / touchdown [N,F] (air_in / ct_in: what air / ct held before the call - the same pointers for device buffers, never restrict)
struct SensorOut {
  int mode;
  float* force; float* torque; int32_t* count;
  float* row; long long row_stride;
  const uint8_t* reset; const float* air_in; const float* ct_in; float* air; float* ct; float* touchdown;
  float threshold, dt;
};

// dynamic LDS: [epb counts | epb * pitch record dwords], pitch = (kmax * kRec) | 1
__global__ __launch_bounds__(kThreads) void contact_sensor_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                                  const rsb_contact* __restrict__ contacts, const int32_t* __restrict__ counts,
                                                                  const FrameList frames, int F, int N, int kmax, int epb, float inv_dt, int flags,
                                                                  const SensorOut s) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const DevModel& m = *model;
  stage_rows(m, rows);
  const long long env0 = (long long)blockIdx.x * epb;
  const int here = (int)min((long long)epb, (long long)N - env0);
  const int per = kmax * kRec, pitch = per | 1;
  uint32_t* cnt = lds;
  uint32_t* recs = lds + epb;
  const uint32_t* src = (const uint32_t*)(contacts + (size_t)env0 * kmax);
  for (int e = threadIdx.x; e < here * per; e += kThreads) {
    const int k = e / per;
    recs[k * pitch + (e - k * per)] = src[e];
  }
  for (int e = threadIdx.x; e < here; e += kThreads) cnt[e] = (uint32_t)min(max(counts[env0 + e], 0), kmax);
  __syncthreads();
  const int el = threadIdx.x / F, fr = threadIdx.x - el * F;
  if (el >= here) return;
  const long long env = env0 + el, idx = env * F + fr;
  const rsb_frame f = frames.f[fr];
  const float* q = gc + (size_t)env * m.nq;
  const float* u = gv + (size_t)env * m.nv;
  Chain c;
  walk_chain<false>(m, rows, q, u, nullptr, s.mode == kObserve, f.body, c, NoJoint{});
  float o[3], pf[3];
  mat3_vec(c.R, f.offset, o);
  for (int k = 0; k < 3; ++k) pf[k] = c.p[k] + o[k];
  float force[3] = {0.f, 0.f, 0.f}, torque[3] = {0.f, 0.f, 0.f}, nf = 0.f, slip = 0.f;
  int owned = 0;
  const bool no_self = (flags & RSB_CONTACT_NO_SELF) != 0;
  const uint32_t* rec = recs + el * pitch;
  const int n = (int)cnt[el];
  for (int k = 0; k < n; ++k, rec += kRec) {
    if ((int)rec[10] != f.body) continue;
    if (no_self && (rec[11] & (RSB_CONTACT_SELF_A | RSB_CONTACT_SELF_B))) continue;
    float pos[3], nrm[3], imp[3], fo[3], r[3], rf[3];
    for (int j = 0; j < 3; ++j) { pos[j] = __uint_as_float(rec[j]); nrm[j] = __uint_as_float(rec[3 + j]); imp[j] = __uint_as_float(rec[6 + j]); }
    for (int j = 0; j < 3; ++j) { fo[j] = imp[j] * inv_dt; r[j] = pos[j] - pf[j]; }
    cross3(r, fo, rf);
    for (int j = 0; j < 3; ++j) { force[j] += fo[j]; torque[j] += rf[j]; }
    nf += dot3(imp, nrm) * inv_dt;
    ++owned;
    if (s.mode == kObserve) {      // the velocity of the body's material point at the record, without its part along the normal
      float d[3], wd[3], v[3], t[3];
      for (int j = 0; j < 3; ++j) d[j] = pos[j] - c.p[j];
      cross3(c.w, d, wd);
      for (int j = 0; j < 3; ++j) v[j] = c.v[j] + wd[j];
      const float vn = dot3(v, nrm);
      for (int j = 0; j < 3; ++j) t[j] = v[j] - vn * nrm[j];
      slip = fmaxf(slip, sqrtf(dot3(t, t)));
    }
  }
  if (flags & RSB_CONTACT_LOCAL) {
    float t[3];
    mat3t_vec(c.R, force, t);
    for (int k = 0; k < 3; ++k) force[k] = t[k];
    mat3t_vec(c.R, torque, t);
    for (int k = 0; k < 3; ++k) torque[k] = t[k];
  }
  const bool contact = nf > s.threshold;
  if (s.mode == kObserve) {
    float* row = s.row + env * s.row_stride + 6 * fr;
    row[0] = contact ? 1.f : 0.f;
    for (int k = 0; k < 3; ++k) row[1 + k] = force[k];
    row[4] = nf;
    row[5] = slip;
  } else if (s.mode == kWrench) {
    if (s.force) for (int k = 0; k < 3; ++k) s.force[idx * 3 + k] = force[k];
    if (s.torque) for (int k = 0; k < 3; ++k) s.torque[idx * 3 + k] = torque[k];
    if (s.count) s.count[idx] = owned;
  } else {
    const float a_old = s.air_in ? s.air_in[idx] : 0.f, c_old = s.ct_in ? s.ct_in[idx] : 0.f;
    float td = 0.f, a = 0.f, ct = 0.f;
    if (s.reset && s.reset[env]) {
    } else if (contact) {
      td = a_old; ct = c_old + s.dt;
    } else {
      a = a_old + s.dt;
    }
    if (s.air) s.air[idx] = a;
    if (s.ct) s.ct[idx] = ct;
    if (s.touchdown) s.touchdown[idx] = td;
  }
}

// the checks the three entry points share (after check_world)
int check_sensor(const rsb_world* w, const char* who, const rsb_frame* frames, int n_frames, int flags) {
  const int st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (flags & ~(RSB_CONTACT_LOCAL | RSB_CONTACT_NO_SELF)) return invalid(who, "unknown flag bits");
  return RSB_OK;
}
int check_threshold(const char* who, float force_threshold) {
  if (!(force_threshold >= 0.f) || !std::isfinite(force_threshold)) return invalid(who, "force_threshold must be finite and not negative");
  return RSB_OK;
}

// the launch all three entry points share
void launch_sensor(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, const SensorOut& s) {
  const int pitch = (w->kmax * kRec) | 1;
  const int epb = std::max(1, std::min(kThreads / n_frames, kRecLdsDwords / (pitch + 1)));
  const size_t lds = (size_t)epb * (pitch + 1) * sizeof(uint32_t);
  hipLaunchKernelGGL(contact_sensor_kernel, dim3(blocks_for((size_t)w->N, (size_t)epb)), dim3(kThreads), lds, stream_of(w), (const DevModel*)w->d_model,
                     (const float*)w->d_gc, (const float*)w->d_gv, (const rsb_contact*)w->d_contacts, (const int32_t*)w->d_count, frame_list(frames, n_frames),
                     n_frames, w->N, w->kmax, epb, (float)(1.0 / w->dt), flags, s);
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_get_body_contact_wrenches(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, float* force, float* torque, int32_t* count, int space) {
  const char* who = "rsb_get_body_contact_wrenches";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_sensor(w, who, frames, n_frames, flags); if (st != RSB_OK) return st;
  if (!force && !torque && !count) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames;
  float *df, *dq, *dc;
  Staged io(w, space);      // (count: int32 rows travel through the staging buffer like floats)
  io.out(df, force, pairs * 3); io.out(dq, torque, pairs * 3); io.out(dc, reinterpret_cast<float*>(count), pairs);
  st = io.begin(); if (st != RSB_OK) return st;
  SensorOut s{};
  s.mode = kWrench; s.force = df; s.torque = dq; s.count = reinterpret_cast<int32_t*>(dc);
  launch_sensor(w, frames, n_frames, flags, s);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_contact_observe(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, float force_threshold, float* out, long long row_stride, int space) {
  const char* who = "rsb_contact_observe";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_sensor(w, who, frames, n_frames, flags); if (st != RSB_OK) return st;
  st = check_threshold(who, force_threshold); if (st != RSB_OK) return st;
  if (!out) return invalid(who, "out must not be NULL");
  const long long width = 6LL * n_frames;
  if (row_stride == 0) row_stride = width;
  if (row_stride < width) return invalid(who, "row_stride " + std::to_string(row_stride) + " is smaller than 6 * n_frames = " + std::to_string(width));
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  float* dout;
  Staged io(w, space);      // RSB_HOST: the rows are staged dense; they go to the caller's stride on the way back, below, not through end()
  io.out(dout, out, N * width);
  st = io.begin(); if (st != RSB_OK) return st;
  hipStream_t strm = stream_of(w);
  SensorOut s{};
  s.mode = kObserve; s.row = dout; s.row_stride = space == RSB_HOST ? width : row_stride; s.threshold = force_threshold;
  launch_sensor(w, frames, n_frames, flags, s);
  HIP_TRY(hipGetLastError());
  if (space == RSB_HOST) {
    const int fs = fault_status(w); if (fs != RSB_OK) return fs;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)row_stride * sizeof(float), dout, (size_t)width * sizeof(float), (size_t)width * sizeof(float), N, hipMemcpyDeviceToHost, strm));
    HIP_TRY(hipStreamSynchronize(strm));
  }
  return RSB_OK;
}

int rsb_contact_timers(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, float force_threshold, float dt, const uint8_t* reset_mask, float* air_time,
                       float* contact_time, float* touchdown, int space) {
  const char* who = "rsb_contact_timers";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_sensor(w, who, frames, n_frames, flags); if (st != RSB_OK) return st;
  st = check_threshold(who, force_threshold); if (st != RSB_OK) return st;
  if (!(dt > 0.f) || !std::isfinite(dt)) return invalid(who, "dt must be positive and finite");
  if (!air_time && !contact_time) return invalid(who, "air_time and contact_time are both NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t pairs = (size_t)w->N * n_frames;
  const uint8_t* dm;
  const float *dai, *dci;
  float *da, *dc, *dt_;
  Staged io(w, space);      // [mask | air in | contact in | air out | contact out | touchdown]: RSB_HOST reads and writes different slices
  io.in(dm, reset_mask, (size_t)w->N); io.in(dai, air_time, pairs); io.in(dci, contact_time, pairs);
  io.out(da, air_time, pairs); io.out(dc, contact_time, pairs); io.out(dt_, touchdown, pairs);
  st = io.begin(); if (st != RSB_OK) return st;
  SensorOut s{};
  s.mode = kTimers; s.reset = dm; s.air_in = dai; s.ct_in = dci; s.air = da; s.ct = dc; s.touchdown = dt_; s.threshold = force_threshold; s.dt = dt;
  launch_sensor(w, frames, n_frames, flags, s);
  HIP_TRY(hipGetLastError());
  return io.end();
}

}  // extern "C"
