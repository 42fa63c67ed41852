// terrain_ray.h — ONE ray against the terrain, for the kernels of rsb_ray_scan.hip (ray_cast_kernel, ray_scan_kernel).  The surface itself stays the
// caller's: the march asks a `gap` callable for z - h at a ray parameter, and the caller's gap calls rsbk::terrain_eval (step_terrain.h) on its
// own map.  This is ray_test_kernel's walk (rsb_terrain_query.hip), statement for statement.  ray_test_kernel itself keeps its own text: written
// over these functions it compiled to another instruction stream (783 instructions for 787, profiles/ray_scan_digests.txt), and that kernel's code is
// pinned.  rsb_ray_cast without flags must give rsb_ray_test's bits; tests/test_gpu_ray_scan.py holds the two together.
//
//   ray_unit      the direction normalised (first by its largest component: the squares neither overflow nor vanish); false for a ray that cannot
//                 be cast - a zero or non-finite direction, a non-finite origin.
//   plane_ray     the infinite plane z = ground_z.
//   heightmap_ray the ray clipped to the part [lo, hi] of [0, max_dist] over the map's footprint (and at or below the highest sample), then walked
//                 cell by cell (Amanatides & Woo 1987), each cell split at its diagonal: z - h is linear on each piece, so it is evaluated at the
//                 piece's ends and the crossing interpolated.  The cell loop runs at most hm_xs + hm_ys times - every pass moves one cell index one
//                 step in a fixed direction inside the grid - and nothing else loops.
// All three return the range along the unit direction, -1 for a miss.
#pragma once

#include <hip/hip_runtime.h>

namespace rsbk {

__device__ __forceinline__ bool ray_unit(float ox, float oy, float oz, float& dx, float& dy, float& dz) {
  const float big = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
  const bool usable = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) && big > 0.f;
  if (!usable) return false;
  dx /= big; dy /= big; dz /= big;                       // (the squares below neither overflow nor vanish)
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  dx /= len; dy /= len; dz /= len;
  return true;
}

__device__ __forceinline__ float plane_ray(float ground_z, float oz, float dz, float max_dist) {
  float hit = -1.f;
  if (oz <= ground_z) hit = 0.f;
  else if (dz < 0.f) { const float s = (ground_z - oz) / dz; if (s <= max_dist) hit = s; }
  return hit;
}

// t: the terrain as a launch describes it (hm_xs, hm_ys, hm_x0, hm_y0, hm_dx, hm_dy, hm_inv_dx, hm_inv_dy, hm_max); gap(s) = z - h at parameter s
template <class T, class G>
__device__ __forceinline__ float heightmap_ray(const T& t, float ox, float oy, float oz, float dx, float dy, float dz, float max_dist, G&& gap) {
  const int xs = t.hm_xs, ys = t.hm_ys;
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
  if (!(meets && lo <= hi)) return -1.f;
  float s = lo, g0 = gap(lo);
  if (g0 <= 0.f) return lo;                              // the origin below the surface (lo = 0), or the side wall
  // grid coordinates u = u0 + s du, v = v0 + s dv; the cell under the ray at lo
  const float u0 = (ox - t.hm_x0) * t.hm_inv_dx, v0 = (oy - t.hm_y0) * t.hm_inv_dy, du = dx * t.hm_inv_dx, dv = dy * t.hm_inv_dy;
  int ix = min((int)fminf(fmaxf(u0 + lo * du, 0.f), (float)(xs - 1)), xs - 2);
  int iy = min((int)fminf(fmaxf(v0 + lo * dv, 0.f), (float)(ys - 1)), ys - 2);
  const int stepx = du > 0.f ? 1 : -1, stepy = dv > 0.f ? 1 : -1;
  const float inf = __int_as_float(0x7f800000);
  float hit = -1.f;
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
  return hit;
}

}  // namespace rsbk
