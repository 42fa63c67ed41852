// rsb_terrain_query.hip — batched terrain height queries, height scans and ray tests from the resident state
// (rsb_get_terrain_height, rsb_height_scan, rsb_ray_test; include/rsb.h).
//
// What HeightMap::getHeight / getNormal and World::rayTest give for one world and one point or ray on the host [RECALL], for all N envs in one call,
// on the world's stream.  Nothing here is shared with the step kernel's instances: these are short kernels of their own, called between two control
// steps.  The chain walk, the argument checks and the staging of the RSB_HOST forms are those of all batched queries (frames_chain.h).  There is ONE
// definition of the surface: every kernel asks rsbk::terrain_eval (step_terrain.h), the function the collider's resolve uses, through a Terrain struct
// that carries the hm_* fields with the values the step launch gives them.  With per-env maps (rsb_set_heightmaps) an env reads its own map
// (hm_index).  terrain_eval clamps the coordinates to the map: no query reads outside it, whatever the caller passes.
//
//   terrain_height_kernel  one lane per (env, point): height and unit normal of the triangle under the point.
//   height_scan_kernel     the hot path: out[env, frame, k] = p_z - h(p_xy + M pattern[k]), p the frame's world position.  Two phases, as
//                          frame_jacobians_kernel: a workgroup takes `ppb` consecutive (env, frame) pairs; (1) one lane per pair walks the support chain
//                          (frames_chain.h) and leaves (p, c, s, map, env, frame) in LDS; (2) all lanes sweep the ppb * P outputs, consecutive lanes
//                          writing consecutive floats.  The pattern is staged in LDS once per workgroup.  A lane's result depends on its (env, frame,
//                          point) alone, so a frame's scan does not depend on which other frames a call lists.
//   ray_test_kernel        one lane per ray.  The ray is clipped to the part [lo, hi] of [0, max_dist] over the map's footprint (and at or below the
//                          highest sample), then walked cell by cell (Amanatides & Woo 1987), each cell split at its diagonal: z - h is linear on each
//                          piece, so it is evaluated at the piece's ends and the crossing interpolated.  The cell loop runs at most hm_xs + hm_ys
//                          times - every pass moves one cell index one step in a fixed direction inside the grid - and nothing else loops.
#include "frames_chain.h"
#include "rsb_world.h"
#include "step_terrain.h"

namespace rsbw {
namespace {

constexpr int kPairRec = 8;          // height scan, per pair in LDS: p 0-2, c 3, s 4, map 5, env 6, frame 7

// the terrain as the step launch describes it (StepArgs' fields of the same names, the same values)
struct Terrain {
  int terrain_type, hm_xs, hm_ys;
  float ground_z, hm_x0, hm_y0, hm_dx, hm_dy, hm_inv_dx, hm_inv_dy, hm_max;
  const float* heights;        // [n_maps][hm_ys][hm_xs]
  const int32_t* hm_index;     // [N] height map of each env (NULL: every env uses map 0)
};

__device__ __forceinline__ const float* map_of(const Terrain& t, int env) {
  const int map = t.hm_index ? t.hm_index[env] : 0;
  return t.heights + (size_t)map * t.hm_xs * t.hm_ys;
}

__global__ __launch_bounds__(kThreads) void terrain_height_kernel(const Terrain t, const float* __restrict__ xy, int P, long long total,
                                                                  float* __restrict__ height, float* __restrict__ normal) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  float h = t.ground_z, n[3] = {0.f, 0.f, 1.f};
  if (t.terrain_type == 1) rsbk::terrain_eval(t, map_of(t, (int)(idx / P)), xy[idx * 2], xy[idx * 2 + 1], h, n);
  if (height) height[idx] = h;
  if (normal) for (int k = 0; k < 3; ++k) normal[idx * 3 + k] = n[k];
}

// dynamic LDS: [nb * kRow model rows | P * 2 pattern | ppb pair records of kPairRec floats]
__global__ __launch_bounds__(kThreads) void height_scan_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const FrameList frames, int F, int N,
                                                               const Terrain t, const float* __restrict__ pattern, int P, int mode, int ppb,
                                                               float* __restrict__ out, long long row_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DevModel& m = *model;
  float* rows = lds;
  float* pat = lds + m.nb * kRow;
  float* recs = pat + 2 * P;
  stage_rows(m, rows);
  for (int k = threadIdx.x; k < 2 * P; k += kThreads) pat[k] = pattern[k];
  __syncthreads();
  const long long pairs = (long long)N * F, pair0 = (long long)blockIdx.x * ppb;
  const int here = (int)min((long long)ppb, pairs - pair0);
  if ((int)threadIdx.x < here) {
    const long long idx = pair0 + threadIdx.x;
    const int env = (int)(idx / F), fr = (int)(idx - (long long)env * F);
    const rsb_frame f = frames.f[fr];
    const float* q = gc + (size_t)env * m.nq;
    Chain c;
    walk_chain<false>(m, rows, q, nullptr, nullptr, false, f.body, c, NoJoint{});
    float o[3];
    mat3_vec(c.R, f.offset, o);
    float* r = recs + threadIdx.x * kPairRec;
    for (int k = 0; k < 3; ++k) r[k] = c.p[k] + o[k];
    float cs = 1.f, sn = 0.f;
    if (mode == RSB_SCAN_YAW) {
      const float hy = sqrtf(c.R[0] * c.R[0] + c.R[3] * c.R[3]);
      if (hy >= 1e-6f) { cs = c.R[0] / hy; sn = c.R[3] / hy; }
    }
    r[3] = cs; r[4] = sn;
    r[5] = __int_as_float(t.hm_index ? t.hm_index[env] : 0);
    r[6] = __int_as_float(env); r[7] = __int_as_float(fr);
  }
  __syncthreads();
  const bool hm = t.terrain_type == 1;
  const size_t map_floats = (size_t)t.hm_xs * t.hm_ys;
  for (int e = threadIdx.x; e < here * P; e += kThreads) {
    const int k = e / P, j = e - k * P;
    const float* r = recs + k * kPairRec;
    const float2 a = reinterpret_cast<const float2*>(pat)[j];      // (8-byte aligned: nb * kRow is a multiple of 4 floats) one ds_read_b64
    const float ax = a.x, ay = a.y;
    const float x = r[0] + (r[3] * ax - r[4] * ay), y = r[1] + (r[4] * ax + r[3] * ay);
    float h = t.ground_z, n[3];
    if (hm) rsbk::terrain_eval(t, t.heights + (size_t)__float_as_int(r[5]) * map_floats, x, y, h, n);
    out[(long long)__float_as_int(r[6]) * row_stride + (long long)__float_as_int(r[7]) * P + j] = r[2] - h;
  }
}

__global__ __launch_bounds__(kThreads) void ray_test_kernel(const Terrain t, const float* __restrict__ origins, const float* __restrict__ directions, int R,
                                                            long long total, float max_dist, float* __restrict__ dist) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const float ox = origins[idx * 3], oy = origins[idx * 3 + 1], oz = origins[idx * 3 + 2];
  float dx = directions[idx * 3], dy = directions[idx * 3 + 1], dz = directions[idx * 3 + 2];
  const float big = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
  const bool usable = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) && big > 0.f;
  if (!usable) { dist[idx] = -1.f; return; }
  dx /= big; dy /= big; dz /= big;                       // (the squares below neither overflow nor vanish)
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  dx /= len; dy /= len; dz /= len;
  float hit = -1.f;
  if (t.terrain_type != 1) {                             // the infinite plane z = ground_z
    if (oz <= t.ground_z) hit = 0.f;
    else if (dz < 0.f) { const float s = (t.ground_z - oz) / dz; if (s <= max_dist) hit = s; }
    dist[idx] = hit;
    return;
  }
  const int xs = t.hm_xs, ys = t.hm_ys;
  const float* heights = map_of(t, (int)(idx / R));
  // [lo, hi]: the part of [0, max_dist] over the footprint [x0, x1] x [y0, y1] ...
  const float x1 = t.hm_x0 + t.hm_dx * (float)(xs - 1), y1 = t.hm_y0 + t.hm_dy * (float)(ys - 1);
  float lo = 0.f, hi = max_dist;
  bool meets = true;
  if (dx != 0.f) { const float a = (t.hm_x0 - ox) / dx, b = (x1 - ox) / dx; lo = fmaxf(lo, fminf(a, b)); hi = fminf(hi, fmaxf(a, b)); }
  else meets = meets && ox >= t.hm_x0 && ox <= x1;
  if (dy != 0.f) { const float a = (t.hm_y0 - oy) / dy, b = (y1 - oy) / dy; lo = fmaxf(lo, fminf(a, b)); hi = fminf(hi, fmaxf(a, b)); }
  else meets = meets && oy >= t.hm_y0 && oy <= y1;
  // ... and at or below a ceiling a little above the highest sample: above it the ray is above the surface.  (Where this moves lo, the ray is above the
  // surface at lo: the side wall can only be hit where lo is still the footprint's.)
  const float top = t.hm_max + 1e-4f * (1.f + fabsf(t.hm_max));
  if (dz > 0.f) hi = fminf(hi, (top - oz) / dz);
  else if (dz < 0.f) lo = fmaxf(lo, (top - oz) / dz);
  else meets = meets && oz <= top;
  if (!(meets && lo <= hi)) { dist[idx] = -1.f; return; }
  const auto gap = [&](float s) {                        // z - h at parameter s
    float h, n[3];
    rsbk::terrain_eval(t, heights, ox + s * dx, oy + s * dy, h, n);
    return oz + s * dz - h;
  };
  float s = lo, g0 = gap(lo);
  if (g0 <= 0.f) { dist[idx] = lo; return; }            // the origin below the surface (lo = 0), or the side wall
  // grid coordinates u = u0 + s du, v = v0 + s dv; the cell under the ray at lo
  const float u0 = (ox - t.hm_x0) * t.hm_inv_dx, v0 = (oy - t.hm_y0) * t.hm_inv_dy, du = dx * t.hm_inv_dx, dv = dy * t.hm_inv_dy;
  int ix = min((int)fminf(fmaxf(u0 + lo * du, 0.f), (float)(xs - 1)), xs - 2);
  int iy = min((int)fminf(fmaxf(v0 + lo * dv, 0.f), (float)(ys - 1)), ys - 2);
  const int stepx = du > 0.f ? 1 : -1, stepy = dv > 0.f ? 1 : -1;
  const float inf = __int_as_float(0x7f800000);
  for (int it = 0; it < xs + ys; ++it) {
    // where the ray leaves cell (ix, iy): from the cell's own borders, not accumulated (fminf drops a NaN of 0 / 0)
    const float sx = du != 0.f ? ((float)(ix + (du > 0.f ? 1 : 0)) - u0) / du : inf;
    const float sy = dv != 0.f ? ((float)(iy + (dv > 0.f ? 1 : 0)) - v0) / dv : inf;
    const float sb = fminf(fminf(sx, sy), hi);
    // the cell's diagonal u - ix = v - iy
    const float sd = du != dv ? ((v0 - (float)iy) - (u0 - (float)ix)) / (du - dv) : -1.f;
    if (sd > s && sd < sb) {
      const float g1 = gap(sd);
      if (g1 <= 0.f) { hit = fminf(fmaxf(s + (sd - s) * (g0 / (g0 - g1)), s), sd); break; }
      s = sd; g0 = g1;
    }
    if (sb > s) {
      const float g1 = gap(sb);
      if (g1 <= 0.f) { hit = fminf(fmaxf(s + (sb - s) * (g0 / (g0 - g1)), s), sb); break; }
      s = sb; g0 = g1;
    }
    if (!(sb < hi)) break;                               // the end of [lo, hi]: a miss
    if (sx <= sy) ix += stepx; else iy += stepy;
    if (ix < 0 || ix > xs - 2 || iy < 0 || iy > ys - 2) break;
  }
  dist[idx] = hit;
}

Terrain terrain_of(const rsb_world* w) {       // as do_integrate fills StepArgs (rsb_world.hip)
  Terrain t{};
  t.terrain_type = w->terrain_type; t.hm_xs = w->hm_xs; t.hm_ys = w->hm_ys; t.ground_z = (float)w->ground_z;
  if (w->terrain_type == 1) {
    const double dx = w->hm_xsize / (w->hm_xs - 1), dy = w->hm_ysize / (w->hm_ys - 1);
    t.hm_x0 = (float)(w->hm_cx - 0.5 * w->hm_xsize); t.hm_y0 = (float)(w->hm_cy - 0.5 * w->hm_ysize);
    t.hm_dx = (float)dx; t.hm_dy = (float)dy; t.hm_inv_dx = (float)(1.0 / dx); t.hm_inv_dy = (float)(1.0 / dy);
    t.hm_max = w->hm_max;
  }
  t.heights = w->d_heights; t.hm_index = w->d_hm_index;
  return t;
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_get_terrain_height(rsb_world* w, const float* xy, int n_points, float* height, float* normal, int space) {
  const char* who = "rsb_get_terrain_height";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!xy) return invalid(who, "xy is NULL");
  if (n_points < 1) return invalid(who, "n_points must be at least 1");
  if (!height && !normal) return invalid(who, "every output is NULL");
  HIP_TRY(hipSetDevice(w->device));
  const size_t total = (size_t)w->N * n_points;
  const float* dxy;
  float *dh, *dn;
  Staged io(w, space);
  io.in(dxy, xy, total * 2); io.out(dh, height, total); io.out(dn, normal, total * 3);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(terrain_height_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, stream_of(w), terrain_of(w), dxy, n_points, (long long)total, dh, dn);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_height_scan(rsb_world* w, const rsb_frame* frames, int n_frames, const float* pattern, int n_points, int mode, float* out, long long row_stride,
                    int space) {
  const char* who = "rsb_height_scan";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!pattern || !out) return invalid(who, "pattern and out must not be NULL");
  if (n_points < 1 || n_points > RSB_MAX_SCAN_POINTS) return invalid(who, "n_points must be 1.." + std::to_string(RSB_MAX_SCAN_POINTS));
  if (mode != RSB_SCAN_WORLD && mode != RSB_SCAN_YAW) return invalid(who, "mode must be RSB_SCAN_WORLD or RSB_SCAN_YAW");
  const long long width = (long long)n_frames * n_points;
  if (row_stride == 0) row_stride = width;
  if (row_stride < width) return invalid(who, "row_stride " + std::to_string(row_stride) + " is smaller than n_frames * n_points = " + std::to_string(width));
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N, pairs = N * n_frames;
  const float* dp;
  float* dout;
  Staged io(w, space);      // RSB_HOST: the scan is staged dense; its rows go to the caller's stride on the way back, below, not through end()
  io.in(dp, pattern, (size_t)n_points * 2); io.out(dout, out, N * width);
  st = io.begin(); if (st != RSB_OK) return st;
  const long long dstride = space == RSB_HOST ? width : row_stride;
  hipStream_t s = stream_of(w);
  const int ppb = std::max(1, std::min(64, (4 * kThreads + n_points - 1) / n_points));      // phase 2 sweeps about four blocks' worth of outputs
  const size_t lds = ((size_t)w->blob.nb * kRow + (size_t)n_points * 2 + (size_t)ppb * kPairRec) * sizeof(float);
  hipLaunchKernelGGL(height_scan_kernel, dim3(blocks_for(pairs, ppb)), dim3(kThreads), lds, s, (const DevModel*)w->d_model, (const float*)w->d_gc,
                     frame_list(frames, n_frames), n_frames, w->N, terrain_of(w), dp, n_points, mode, ppb, dout, dstride);
  HIP_TRY(hipGetLastError());
  if (space == RSB_HOST) {
    const int fs = fault_status(w); if (fs != RSB_OK) return fs;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)row_stride * sizeof(float), dout, (size_t)width * sizeof(float), (size_t)width * sizeof(float), N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return RSB_OK;
}

int rsb_ray_test(rsb_world* w, const float* origins, const float* directions, int n_rays, float max_dist, float* dist, int space) {
  const char* who = "rsb_ray_test";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!origins || !directions) return invalid(who, "origins and directions must not be NULL");
  if (!dist) return invalid(who, "every output is NULL");
  if (n_rays < 1) return invalid(who, "n_rays must be at least 1");
  if (!(max_dist > 0.f) || !std::isfinite(max_dist)) return invalid(who, "max_dist must be positive and finite");
  HIP_TRY(hipSetDevice(w->device));
  const size_t total = (size_t)w->N * n_rays;
  const float *dor, *ddi;
  float* dd;
  Staged io(w, space);
  io.in(dor, origins, total * 3); io.in(ddi, directions, total * 3); io.out(dd, dist, total);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(ray_test_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, stream_of(w), terrain_of(w), dor, ddi, n_rays, (long long)total, max_dist, dd);
  HIP_TRY(hipGetLastError());
  return io.end();
}

}  // extern "C"
