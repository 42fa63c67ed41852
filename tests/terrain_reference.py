"""An independent fp64 reference of the sphere x height-map collider, for tests/test_terrain_contact_reference.py (the oracle) and
tests/test_gpu_terrain_contact.py (the kernel).  Plain numpy; no code and no structure of oracle/rsb_oracle.c or step_terrain.h:

  mesh ............ every triangle of the map (each cell split along (ix, iy)-(ix+1, iy+1)); it ends at the border.
  closest point ... per triangle: the foot of the perpendicular on its plane if the signed areas put it inside, else the nearest point of the
                    three edges (each a clamped segment) - not a Voronoi-region cascade; then the minimum over the WHOLE map, no cell window.
  height .......... barycentric weights of the triangle under (x, y), coordinates clamped to the footprint.
  verdict ......... tie-robust (equally close features have unrelated normals, so normals are never compared feature by feature); for a
                    reported contact (position, normal, depth) of a sphere (centre c, radius r):
                      (a) |normal| = 1 and position = c - r normal;
                      (b) the terrain point p = position + depth normal lies on the mesh (brute-force distance <= bar);
                      (c) no mesh point is closer: |p - c| <= D_min (1 + tie) + bar;
                      (d) reported <=> D_min < r; placements with |D_min - r| <= bar are left out of (d) only.

The conventions the collider documents, restated here and nowhere taken from its code:
  * centre inside the footprint (border included) and above the surface: the closest feature; for r <= min(dx, dy) over the whole mesh, for a
    larger sphere over the documented 3 x 3 window - on an axis whose bounding span reaches 3 cells, the centre's cell +- 1, clamped to the map;
  * centre inside the footprint, at or below the surface: depth = r - (z - h) n_z, n = the face normal of the triangle under the centre;
  * centre beyond the footprint: depth = r - (z - h(clamped x, clamped y)), normal = (0, 0, 1).

Also here: the "rake" (one floating link carrying 24 spheres) and the placement families both tiers use.
"""
import numpy as np

N_SPHERES = 24
REGIME_NAMES = ("above, r <= cell (whole mesh)", "above, r > cell (3 x 3 window)", "at or below the surface", "beyond the footprint")
FAMILIES = ("generic interior", "grid line in x", "grid line in y", "grid node", "cell diagonal", "border cell, overhanging", "beyond the border",
            "exactly on the near border")


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class Grid:
    """A height map as a triangle soup.  heights [ys, xs] (rounded to float32: what both colliders store)."""

    def __init__(self, heights, xsize, ysize, cx, cy):
        self.h32 = np.ascontiguousarray(heights, np.float32)
        self.h = self.h32.astype(np.float64)
        self.ys, self.xs = self.h.shape
        self.xsize, self.ysize, self.cx, self.cy = float(xsize), float(ysize), float(cx), float(cy)
        self.x0, self.y0 = cx - 0.5 * xsize, cy - 0.5 * ysize
        self.x1, self.y1 = self.x0 + xsize, self.y0 + ysize
        self.dx, self.dy = xsize / (self.xs - 1), ysize / (self.ys - 1)
        self.hmax = float(self.h.max())
        self._memo = {}
        X, Y = np.meshgrid(self.x0 + self.dx * np.arange(self.xs), self.y0 + self.dy * np.arange(self.ys))
        V = np.stack([X, Y, self.h], axis=-1)
        v00, v10, v01, v11 = V[:-1, :-1], V[:-1, 1:], V[1:, :-1], V[1:, 1:]
        flat = lambda a: a.reshape(-1, 3)      # noqa: E731
        self.A = np.concatenate([flat(v00), flat(v00)])
        self.B = np.concatenate([flat(v10), flat(v11)])
        self.C = np.concatenate([flat(v11), flat(v01)])
        iy, ix = np.meshgrid(np.arange(self.ys - 1), np.arange(self.xs - 1), indexing="ij")
        self.tri_ix, self.tri_iy = np.tile(ix.ravel(), 2), np.tile(iy.ravel(), 2)
        n = np.cross(self.B - self.A, self.C - self.A)
        self.Nu = n / np.linalg.norm(n, axis=1, keepdims=True)      # unit face normals, all pointing up
        assert (self.Nu[:, 2] > 0).all() and len(self.A) == 2 * (self.xs - 1) * (self.ys - 1)

    def args(self):
        return self.xs, self.ys, self.xsize, self.ysize, self.cx, self.cy, self.h32

    # ---- the surface under (x, y) ----
    def under(self, x, y):
        """-> (height, unit face normal [.., 3], distance of (x, y) from the nearest cell edge or diagonal in grid units), coordinates clamped"""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        u = np.clip((x - self.x0) / self.dx, 0.0, self.xs - 1.0)
        v = np.clip((y - self.y0) / self.dy, 0.0, self.ys - 1.0)
        iu = np.minimum(u.astype(int), self.xs - 2)
        iv = np.minimum(v.astype(int), self.ys - 2)
        a, b = u - iu, v - iv
        h00, h10, h01, h11 = self.h[iv, iu], self.h[iv, iu + 1], self.h[iv + 1, iu], self.h[iv + 1, iu + 1]
        low = a >= b
        # barycentric weights of (v00, v10, v11) resp. (v00, v11, v01)
        h = np.where(low, (1 - a) * h00 + (a - b) * h10 + b * h11, (1 - b) * h00 + a * h11 + (b - a) * h01)
        t = np.where(low, 0, (self.xs - 1) * (self.ys - 1)) + iv * (self.xs - 1) + iu
        edge = np.minimum.reduce([a, 1 - a, b, 1 - b, np.abs(a - b)])
        return h, self.Nu[t], edge

    def inside(self, x, y):
        return (x >= self.x0) & (x <= self.x1) & (y >= self.y0) & (y <= self.y1)

    # ---- brute force ----
    def closest(self, P, window=None, chunk=192):
        """P [M, 3] -> (distance [M], closest mesh point [M, 3]); window = (ix0, ix1, iy0, iy1) int arrays [M]: only triangles of those cells."""
        P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
        key = (P.tobytes(), None if window is None else b"".join(np.ascontiguousarray(w, np.int64).tobytes() for w in window))
        if key in self._memo:      # (the three lane mappings of the device tier ask for the same points)
            return tuple(a.copy() for a in self._memo[key])
        D, Q = np.empty(len(P)), np.empty((len(P), 3))
        for s in range(0, len(P), chunk):
            e = min(s + chunk, len(P))
            q = closest_on_triangles(P[s:e], self.A, self.B, self.C, self.Nu)
            d = np.linalg.norm(q - P[s:e, None, :], axis=-1)
            if window is not None:
                ix0, ix1, iy0, iy1 = (w[s:e, None] for w in window)
                keep = (self.tri_ix[None] >= ix0) & (self.tri_ix[None] <= ix1) & (self.tri_iy[None] >= iy0) & (self.tri_iy[None] <= iy1)
                d = np.where(keep, d, np.inf)
            k = d.argmin(axis=1)
            D[s:e], Q[s:e] = d[np.arange(e - s), k], q[np.arange(e - s), k]
        self._memo[key] = (D.copy(), Q.copy())
        return D, Q

    def window(self, c, r):
        """The documented window of a sphere larger than a cell: per axis the cells its bounding span overlaps; where the span reaches 3 cells,
        the centre's cell +- 1; clamped to the map.  -> (ix0, ix1, iy0, iy1), floor_margin (distance of a deciding quotient from an integer)"""
        out, margin = [], np.full(len(c), np.inf)
        for k, (o, d, n) in enumerate(((self.x0, self.dx, self.xs), (self.y0, self.dy, self.ys))):
            lo, hi, mid = (c[:, k] - r - o) / d, (c[:, k] + r - o) / d, (c[:, k] - o) / d
            i0, i1, ic = np.floor(lo).astype(int), np.floor(hi).astype(int), np.floor(mid).astype(int)
            wide = i1 - i0 >= 3
            i0, i1 = np.where(wide, ic - 1, i0), np.where(wide, ic + 1, i1)
            for g in (lo, hi, mid):
                margin = np.minimum(margin, np.abs(g - np.round(g)))
            i0, i1 = np.maximum(i0, 0), np.minimum(i1, n - 2)
            out += [i0, i1]
        return tuple(out), margin


def closest_on_triangles(P, A, B, C, Nu):
    """P [M, 3] x triangles [T, 3] -> closest points [M, T, 3]"""
    Pm = P[:, None, :]
    s = ((Pm - A[None]) * Nu[None]).sum(-1)
    F = Pm - s[..., None] * Nu[None]                      # foot of the perpendicular on each triangle's plane

    def area(U, V):                                        # signed area of (U, V, F) seen from above the face: ((V - U) x (F - U)) . n
        m = np.cross(Nu, V - U)                            # = (n x (V - U)) . (P - U), because n x (V - U) lies in the plane
        return ((Pm - U[None]) * m[None]).sum(-1)

    inside = (area(A, B) >= 0) & (area(B, C) >= 0) & (area(C, A) >= 0)
    best, bd = None, None
    for U, V in ((A, B), (B, C), (C, A)):
        e = (V - U)[None]
        t = np.clip(((Pm - U[None]) * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
        q = U[None] + t[..., None] * e
        d = ((q - Pm) ** 2).sum(-1)
        if best is None:
            best, bd = q, d
        else:
            take = d < bd
            best, bd = np.where(take[..., None], q, best), np.where(take, d, bd)
    return np.where(inside[..., None], F, best)


# ---- the verdict ----------------------------------------------------------------------------------------------------------------------------
def verdict(grid, c, r, reported, position, normal, depth, tie, bar, unit_tol, exact=None, floor_margin=1e-6):
    """One grid, M placements (centres c [M, 3], radii r [M]) and what a collider reported for them (reported [M] bool; position, normal
    [M, 3], depth [M]: read only where reported).  -> dict of per-placement arrays:
      regime ...... 0..3 (REGIME_NAMES);  excluded: left out of (d) / of the regime's check (a rounding-sized margin decides);  ref_hit
      bad ......... the placement fails its check;  why: text of the first failure
      e_unit, e_pos (a);  e_mesh (b);  e_excess (c, = |p - c| - D_min (1 + tie));  e_depth (|depth - reference depth|)
    Regimes 2 and 3 are closed forms: depth and normal are compared with bar directly.
    exact [M] bool: the centre is the same number on both sides (a sphere at the base position): only such a centre may sit ON the near border."""
    c, r = np.asarray(c, np.float64), np.asarray(r, np.float64)
    M = len(c)
    h, nface, edge = grid.under(c[:, 0], c[:, 1])
    inside = grid.inside(c[:, 0], c[:, 1])
    big = r > min(grid.dx, grid.dy)
    regime = np.where(~inside, 3, np.where(c[:, 2] <= h, 2, np.where(big, 1, 0)))
    excluded = np.zeros(M, bool)
    # a border is an inside / outside tie unless the centre is exactly on the NEAR one (x0 + xsize vs x0 + dx (xs - 1) differ in fp32)
    for k, (lo, hi) in enumerate(((grid.x0, grid.x1), (grid.y0, grid.y1))):
        excluded |= (np.abs(c[:, k] - lo) <= 10 * bar) & ~((c[:, k] == lo) & (np.zeros(M, bool) if exact is None else exact))
        excluded |= np.abs(c[:, k] - hi) <= 10 * bar
    excluded |= inside & (np.abs(c[:, 2] - h) <= bar)                      # above / below the surface is a tie
    excluded |= (regime == 2) & (edge < 1e-3)                              # the triangle under the centre is a tie
    ref_depth, ref_hit = np.zeros(M), np.zeros(M, bool)
    D = np.full(M, np.nan)
    out = {k: np.zeros(M) for k in ("e_unit", "e_pos", "e_mesh", "e_excess", "e_depth")}
    bad, why = np.zeros(M, bool), np.array([""] * M, dtype=object)
    rep = np.asarray(reported, bool)
    pos, nrm, dep = (np.where(rep.reshape((M,) + (1,) * (np.ndim(a) - 1)), a, 0.0) for a in (position, normal, depth))

    def fail(sel, text):
        new = sel & ~bad
        why[new] = text
        bad[:] |= sel

    out["e_unit"] = np.where(rep, np.abs(np.linalg.norm(nrm, axis=1) - 1.0), 0.0)
    out["e_pos"] = np.where(rep, np.abs(pos - (c - r[:, None] * nrm)).max(axis=1), 0.0)
    fail(rep & (out["e_unit"] > unit_tol), "(a) the normal is not a unit vector")
    fail(rep & (out["e_pos"] > bar), "(a) position != c - r normal")

    m = regime <= 1
    if m.any():
        win, wmargin = grid.window(c, r)
        wsel = None
        if (regime == 1).any():
            excluded |= (regime == 1) & (wmargin <= floor_margin)                   # a floor() of the window rule is a tie
            full = (np.zeros(M, int), np.full(M, grid.xs - 2), np.zeros(M, int), np.full(M, grid.ys - 2))
            wsel = tuple(np.where(regime == 1, w, f)[m] for w, f in zip(win, full))
        D[m], _ = grid.closest(c[m], wsel)
        ref_hit[m] = D[m] < r[m]
        ref_depth[m] = r[m] - D[m]
        near = m & (np.abs(D - r) <= bar)
        mr = m & rep
        if mr.any():
            p = pos + dep[:, None] * nrm
            wr = None if wsel is None else tuple(np.where(regime == 1, w, f)[mr] for w, f in zip(win, full))
            out["e_mesh"][mr], _ = grid.closest(p[mr], wr)
            out["e_excess"][mr] = np.linalg.norm(p[mr] - c[mr], axis=1) - D[mr] * (1.0 + tie)
            out["e_depth"][mr] = np.abs(dep[mr] - ref_depth[mr])
            fail(mr & ~excluded & (out["e_mesh"] > bar), "(b) the terrain point is off the mesh")
            fail(mr & ~excluded & (out["e_excess"] > bar), "(c) a mesh point is closer")
        fail(m & ~excluded & ~near & (rep != ref_hit), "(d) reported <=> D_min < r")
        excluded |= near
    m = regime == 2
    if m.any():
        ref_depth[m] = r[m] - (c[m, 2] - h[m]) * nface[m, 2]
        ref_hit[m] = True
        fail(m & ~excluded & ~rep, "at or below the surface, but nothing reported")
        mr = m & rep
        out["e_depth"][mr] = np.abs(dep[mr] - ref_depth[mr])
        fail(mr & ~excluded & (out["e_depth"] > bar), "below the surface: depth != r - (z - h) n_z")
        fail(mr & ~excluded & (np.abs(nrm - nface).max(axis=1) > bar), "below the surface: normal != the face normal under the centre")
    m = regime == 3
    if m.any():
        ref_depth[m] = r[m] - (c[m, 2] - h[m])
        ref_hit[m] = ref_depth[m] > 0.0
        near = m & (np.abs(ref_depth) <= bar)
        fail(m & ~excluded & ~near & (rep != ref_hit), "beyond the footprint: reported <=> r - (z - h(clamped)) > 0")
        mr = m & rep
        out["e_depth"][mr] = np.abs(dep[mr] - ref_depth[mr])
        fail(mr & ~excluded & (out["e_depth"] > bar), "beyond the footprint: depth != r - (z - h(clamped))")
        fail(mr & ~excluded & (np.abs(nrm - np.array([0.0, 0.0, 1.0])).max(axis=1) > bar), "beyond the footprint: normal != z")
        excluded |= near
    out.update(regime=regime, excluded=excluded, ref_hit=ref_hit, ref_depth=ref_depth, bad=bad, why=why, D=D)
    return out


class Tally:
    """worst value per quantity and regime, and the excluded share, over many verdicts"""

    def __init__(self):
        self.n = np.zeros(4, int); self.excl = np.zeros(4, int); self.hits = np.zeros(4, int)
        self.worst = {k: np.zeros(4) for k in ("e_unit", "e_pos", "e_mesh", "e_excess", "e_depth")}
        self.failures = []

    def add(self, v, label=""):
        for g in range(4):
            m = v["regime"] == g
            self.n[g] += m.sum(); self.excl[g] += (m & v["excluded"]).sum(); self.hits[g] += (m & v["ref_hit"]).sum()
            ok = m & ~v["excluded"]
            for k in self.worst:
                if ok.any():
                    self.worst[k][g] = max(self.worst[k][g], float(v[k][ok].max()))
        for i in np.nonzero(v["bad"])[0]:
            self.failures.append((label, int(i), REGIME_NAMES[v["regime"][i]], v["why"][i]))

    def excluded_share(self):
        return self.excl.sum() / max(self.n.sum(), 1)

    def lines(self):
        out = []
        for g in range(4):
            w = self.worst
            out.append(f"{REGIME_NAMES[g]:<34} n = {self.n[g]:6d} (hits {self.hits[g]:6d}, excluded {self.excl[g]:4d})  off-mesh {w['e_mesh'][g]:.2e}  "
                       f"distance excess {w['e_excess'][g]:+.2e}  depth error {w['e_depth'][g]:.2e}  |n| - 1 {w['e_unit'][g]:.1e}  position {w['e_pos'][g]:.1e}")
        out.append(f"excluded share {self.excluded_share():.4%} of {self.n.sum()} placements")
        return out


# ---- maps -----------------------------------------------------------------------------------------------------------------------------------
def random_map(xs, ys, xsize, ysize, cx, cy, amplitude, seed, offset=0.0):
    """heights uniform in +- amplitude x the smaller cell size (so amplitude 0.8 gives slopes up to 1.6 across a cell), + offset"""
    cell = min(xsize / (xs - 1), ysize / (ys - 1))
    h = np.random.default_rng(seed).uniform(-amplitude * cell, amplitude * cell, (ys, xs)) + offset
    return Grid(h, xsize, ysize, cx, cy)


def wall_map():
    """5 x 5 samples over 2 m x 2 m, flat except a last column 1.5 m high: the outermost triangles rise steeply towards the border x = 1"""
    h = np.zeros((5, 5)); h[:, 4] = 1.5
    return Grid(h, 2.0, 2.0, 0.0, 0.0)


def corrugated_map(kind, xs=13, ys=11, cell=0.25, rise=0.15):
    """V-valleys (and the ridges between them) one cell apart: along x (heights alternate from row to row), along y, or along the cells' diagonals
    (heights alternate with ix - iy: every diagonal edge is level, the valley lines are diagonals)"""
    iy, ix = np.meshgrid(np.arange(ys), np.arange(xs), indexing="ij")
    k = {"x": iy, "y": ix, "diag": ix - iy}[kind]
    return Grid(rise * (k % 2), cell * (xs - 1), cell * (ys - 1), 0.25, -0.25)


def ridge_map(along, xs=9, ys=7, cell=0.25, height=0.15):
    """one straight tent ridge through the middle of a flat map, along y (a raised column) or along x (a raised row)"""
    h = np.zeros((ys, xs))
    if along == "y":
        h[:, xs // 2] = height
    else:
        h[ys // 2, :] = height
    return Grid(h, cell * (xs - 1), cell * (ys - 1), 0.0, 0.0)


# ---- the second flank -----------------------------------------------------------------------------------------------------------------------
def second_flank_verdict(grid, c, r, first, n1, rep2, pos2, nrm2, dep2, angle, tie, bar, unit_tol, ang_tol=1e-4):
    """The reference set of a sphere: every triangle's closest point that penetrates (d < r), has the centre on the triangle's outer side and whose
    direction is at least `angle` (rad) from the first contact's normal n1 (the reported one).  A second contact is reported iff the set is not
    empty (and the first contact is: `first`); its point is on the mesh, is some qualifying triangle's closest point and is within tie + bar of the
    set's minimum.  A triangle whose qualification margins are inside bar (ang_tol for the angle) may be in or out; a placement whose set is
    empty or not depending on those is excluded.  -> dict(bad, why, excluded, expected, e_mesh, e_excess, e_point)"""
    M = len(c)
    q = closest_on_triangles(c, grid.A, grid.B, grid.C, grid.Nu)
    v = c[:, None, :] - q
    d = np.linalg.norm(v, axis=-1)
    m1 = r[:, None] - d
    m2 = ((c[:, None, :] - grid.A[None]) * grid.Nu[None]).sum(-1)
    cosang = np.clip((v * n1[:, None, :]).sum(-1) / np.maximum(d, 1e-300), -1.0, 1.0)
    m3 = np.arccos(cosang) - angle
    sure = (m1 > bar) & (m2 > bar) & (m3 > ang_tol) & first[:, None]
    maybe = ~((m1 < -bar) | (m2 < -bar) | (m3 < -ang_tol)) & first[:, None]
    has_sure, has_maybe = sure.any(1), maybe.any(1)
    excluded = has_maybe & ~has_sure
    bad, why = np.zeros(M, bool), np.array([""] * M, dtype=object)

    def fail(sel, text):
        why[sel & ~bad] = text
        bad[:] |= sel

    rep2 = np.asarray(rep2, bool)
    fail(has_sure & ~rep2, "a second flank qualifies, none reported")
    fail(~has_maybe & rep2, "a second contact reported, no flank qualifies")
    out = dict(e_mesh=np.zeros(M), e_excess=np.zeros(M), e_point=np.zeros(M))
    mr = rep2 & has_maybe
    if mr.any():
        fail(mr & (np.abs(np.linalg.norm(nrm2, axis=1) - 1.0) > unit_tol), "(a) the second normal is not a unit vector")
        fail(mr & (np.abs(pos2 - (c - r[:, None] * nrm2)).max(axis=1) > bar), "(a) second position != c - r normal")
        p = pos2 + dep2[:, None] * nrm2
        out["e_mesh"][mr], _ = grid.closest(p[mr])
        dp = np.linalg.norm(q - p[:, None, :], axis=-1)
        out["e_point"][mr] = np.where(maybe, dp, np.inf).min(axis=1)[mr]
        dmin = np.where(has_sure, np.where(sure, d, np.inf).min(axis=1), np.where(maybe, d, np.inf).min(axis=1))
        out["e_excess"][mr] = (np.linalg.norm(p - c, axis=1) - dmin * (1.0 + tie))[mr]
        low = np.where(maybe, d, np.inf).min(axis=1) - np.linalg.norm(p - c, axis=1)
        fail(mr & (out["e_mesh"] > bar), "the second terrain point is off the mesh")
        fail(mr & (out["e_point"] > bar), "the second terrain point is no qualifying triangle's closest point")
        fail(mr & (out["e_excess"] > bar), "a qualifying point of another flank is closer")
        fail(mr & (low > bar), "the second contact is closer than every qualifying point")
    out.update(bad=bad, why=why, excluded=excluded, expected=has_sure)
    return out


# ---- the capsule's barrel -------------------------------------------------------------------------------------------------------------------
def capsule_reference(grid, a, b, r, samples=4001):
    """depth r - D_min of `samples` points of the axis segment a .. b through the brute force -> (d*, depth at a, depth at b); every sample must be
    inside the footprint and above the surface (the caller's placements are)"""
    t = np.linspace(0.0, 1.0, samples)[:, None]
    P = a[None] * (1.0 - t) + b[None] * t
    h, _, _ = grid.under(P[:, 0], P[:, 1])
    assert grid.inside(P[:, 0], P[:, 1]).all() and (P[:, 2] > h).all()
    D, _ = grid.closest(P, chunk=4096)
    dep = r - D
    return float(dep.max()), float(dep[0]), float(dep[-1])


def point_segment_distance(p, a, b):
    e = b - a
    t = np.clip(((p - a) * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
    return np.linalg.norm(a + t[..., None] * e - p, axis=-1)


# ---- the rake -------------------------------------------------------------------------------------------------------------------------------
def rake_urdf(offsets, radii, mass=2.0):
    """common.sphere_urdf's pattern with one <collision> per sphere; repr() round-trips the doubles"""
    cols = "".join(f'    <collision><origin xyz="{o[0]!r} {o[1]!r} {o[2]!r}"/><geometry><sphere radius="{float(r)!r}"/></geometry></collision>\n'
                   for o, r in zip(np.asarray(offsets, np.float64).tolist(), radii))
    i = 0.4 * mass * 0.3 * 0.3
    return (f'<?xml version="1.0"?>\n<robot name="rake">\n  <link name="rake">\n    <inertial><origin xyz="0 0 0"/><mass value="{mass}"/>\n'
            f'      <inertia ixx="{i}" ixy="0" ixz="0" iyy="{i}" iyz="0" izz="{i}"/></inertial>\n{cols}  </link>\n</robot>\n')


def is_raised(i):
    return i % 3 == 2      # 8 of 24, interleaved with the 16 that may touch


def sphere_centres(q, offsets):
    """world centres of the spheres for a base state q = (p, quaternion w x y z), fp64; the quaternion is normalised first"""
    q = np.asarray(q, np.float64)
    return q[:3] + np.asarray(offsets, np.float64) @ quat_to_rot(q[3:7] / np.linalg.norm(q[3:7])).T


def _snap(x, bits=12):
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


class RakeDesign:
    """offsets [24, 3], radii [24], family [24] (index into FAMILIES), q [7] (fp64; position and quaternion exact in float32), below [24] and
    raised [24] bool, mode"""


def design_rake(grid, rng, r_lo, r_hi, mode="interior", generic_only=False, reach=0.45, raised_gap=(0.02, 0.25), raised_fn=None, allow_below=True,
                clearance=(0.02, 1.3)):
    """Draws a base pose (full yaw, tilt <= 0.5 rad) over `grid` and 24 sphere offsets such that, at that pose, each sphere sits in its placement
    family at a drawn clearance (z - h) / r in 0.02 .. 1.3 above the surface under it (every 8th or so generic one at -0.8 .. -0.02, centre below
    the surface), the 8 raised ones above the map's highest sample.  Sphere 0 has offset 0: its centre is the base position, exact on both sides.
    mode: "interior" | "edge" (base within 0.3 m of a border) | "on_border" (base exactly on the near border in x, in y or on the near corner)."""
    g = grid
    is_raised = raised_fn or globals()["is_raised"]
    for _attempt in range(200):
        yaw, tilt, tdir = rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 0.5), rng.uniform(-np.pi, np.pi)
        qy = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
        qt = np.array([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(tdir), np.sin(tilt / 2) * np.sin(tdir), 0.0])
        quat = np.array([qy[0] * qt[0] - qy[3] * qt[3], qy[0] * qt[1] - qy[3] * qt[2], qy[0] * qt[2] + qy[3] * qt[1], qy[0] * qt[3] + qy[3] * qt[0]])
        quat = quat.astype(np.float32).astype(np.float64)
        R = quat_to_rot(quat / np.linalg.norm(quat))
        # base xy
        if mode == "on_border":
            which = rng.integers(0, 3)
            px = g.x0 if which != 1 else rng.uniform(g.x0, g.x1)
            py = g.y0 if which != 0 else rng.uniform(g.y0, g.y1)
        elif mode == "edge":
            px, py = rng.uniform(g.x0, g.x1), rng.uniform(g.y0, g.y1)
            side = rng.integers(0, 4)
            d = rng.uniform(0.02, 0.3)
            if side == 0: px = min(g.x0 + d, g.x1)
            elif side == 1: px = max(g.x1 - d, g.x0)
            elif side == 2: py = min(g.y0 + d, g.y1)
            else: py = max(g.y1 - d, g.y0)
        else:
            px, py = rng.uniform(g.x0 + 0.3 * g.dx, g.x1 - 0.3 * g.dx), rng.uniform(g.y0 + 0.3 * g.dy, g.y1 - 0.3 * g.dy)
        px, py = float(_snap(px)), float(_snap(py))
        if mode == "on_border":
            px, py = (g.x0 if which != 1 else px), (g.y0 if which != 0 else py)
        radii = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), N_SPHERES))
        cw, fam, below = np.zeros((N_SPHERES, 3)), np.zeros(N_SPHERES, int), np.zeros(N_SPHERES, bool)
        ok = True
        for i in range(N_SPHERES):
            placed = False
            for _try in range(40):
                if i == 0:
                    f, x, y = (7 if mode == "on_border" else 0), px, py
                else:
                    f = 0 if generic_only else int(rng.integers(0, 7))
                    got = _family_xy(g, rng, f, px, py, reach if not is_raised(i) else 0.3, radii[i])
                    if got is None:
                        f = 0
                        got = _family_xy(g, rng, 0, px, py, reach if not is_raised(i) else 0.3, radii[i])
                        if got is None:
                            f = 6
                            got = _family_xy(g, rng, 6, px, py, reach if not is_raised(i) else 0.3, radii[i])
                            if got is None:
                                continue
                    x, y = got
                h, _, edge = g.under(x, y)
                if is_raised(i):
                    if i > 0 and radii[i] > 0.1 and r_lo <= 0.1:
                        radii[i] = rng.uniform(r_lo, min(0.1, r_hi))
                    z = g.hmax + radii[i] + rng.uniform(*raised_gap)
                    bel = False
                else:
                    bel = allow_below and (f == 0) and (edge >= 2e-3) and bool(g.inside(x, y)) and rng.uniform() < 0.2
                    z = h + radii[i] * (rng.uniform(-0.8, -0.02) if bel else rng.uniform(*clearance))
                if i == 0:
                    pz = float(np.float32(z)); z = pz
                if np.linalg.norm([x - px, y - py, z - pz]) <= 0.6:
                    cw[i], fam[i], below[i], placed = (x, y, z), f, bel, True
                    break
                if i == 0:
                    break
            if not placed:
                ok = False
                break
        if not ok:
            continue
        d = RakeDesign()
        p = np.array([px, py, pz])
        d.offsets = (cw - p) @ R      # R^T (cw - p), row-wise
        d.offsets[0] = 0.0
        d.radii, d.family, d.below = radii, fam, below
        d.raised = np.array([bool(is_raised(i)) for i in range(N_SPHERES)])
        d.q = np.r_[p, quat]
        d.mode = mode
        return d
    raise RuntimeError("no rake fits this map")


def variant_pose(grid, d, rng, offsets, radii, bar, floor_margin, limit=2.9, tries=60, max_hits=16, regime0_only=False):
    """the design pose moved by whole cells (placements on lines, nodes and diagonals stay there) and a little in z, such that no placement is a
    tie of the reference's and at most 16 spheres touch; float32-exact.  None if the draws run out."""
    exact = np.arange(len(radii)) == 0
    zero = np.zeros(len(radii))
    for _ in range(tries):
        q = d.q.copy()
        q[0] += rng.integers(-1, 2) * grid.dx
        q[1] += rng.integers(-1, 2) * grid.dy
        q[2] = np.float32(q[2] + rng.uniform(-0.05, 0.12))
        if np.abs(q[:2]).max() > limit or np.array_equal(q[:3], d.q[:3]):
            continue
        v = verdict(grid, sphere_centres(q, offsets), radii, zero > 1, np.zeros((len(radii), 3)), np.zeros((len(radii), 3)), zero, tie=0.0, bar=bar,
                    unit_tol=1.0, exact=exact, floor_margin=floor_margin)
        if regime0_only and (v["regime"] != 0).any():
            continue
        if not v["excluded"].any() and v["ref_hit"].sum() <= max_hits:
            return q
    return None


def _family_xy(g, rng, f, px, py, reach, r):
    """a point of family f within `reach` of (px, py), or None if the family has none there"""
    def in_reach(x, y):
        return (x - px) ** 2 + (y - py) ** 2 <= reach * reach

    def generic(axis_lo, axis_hi, o, d, n):
        # a coordinate strictly inside the footprint and >= 2e-3 grid units from every grid line
        for _ in range(20):
            v = rng.uniform(axis_lo, axis_hi)
            u = (v - o) / d
            if 0 < u < n - 1 and 2e-3 <= u - np.floor(u) <= 1 - 2e-3:
                return v
        return None

    def lines(o, d, n, centre):
        k = np.arange(1, n - 1)      # (interior lines: a centre computed as p + R l lands on either side of a border line)
        return k[np.abs(o + k * d - centre) < reach]

    for _ in range(20):
        if f in (0, 5):
            x, y = generic(px - reach, px + reach, g.x0, g.dx, g.xs), generic(py - reach, py + reach, g.y0, g.dy, g.ys)
            if x is None or y is None:
                return None
            if f == 5:      # pull one coordinate to within r of a border, inside
                side, u = rng.integers(0, 4), rng.uniform(0.05, 0.9) * r
                if side == 0: x = g.x0 + u
                elif side == 1: x = g.x1 - u
                elif side == 2: y = g.y0 + u
                else: y = g.y1 - u
                if not (g.x0 < x < g.x1 and g.y0 < y < g.y1):
                    continue
            else:
                a, b = (x - g.x0) / g.dx % 1.0, (y - g.y0) / g.dy % 1.0
                if abs(a - b) < 2e-3:
                    continue
        elif f in (1, 2, 3):
            kx, ky = lines(g.x0, g.dx, g.xs, px), lines(g.y0, g.dy, g.ys, py)
            x = g.x0 + g.dx * rng.choice(kx) if f in (1, 3) and len(kx) else generic(px - reach, px + reach, g.x0, g.dx, g.xs)
            y = g.y0 + g.dy * rng.choice(ky) if f in (2, 3) and len(ky) else generic(py - reach, py + reach, g.y0, g.dy, g.ys)
            if x is None or y is None or (f in (1, 3) and not len(kx)) or (f in (2, 3) and not len(ky)):
                return None
            # (a line coinciding with the far border is an inside / outside tie in fp32: the near border and interior lines only)
            if (f in (1, 3) and x >= g.x1) or (f in (2, 3) and y >= g.y1):
                continue
        elif f == 4:
            iu, iv = int(np.floor((px + rng.uniform(-reach, reach) - g.x0) / g.dx)), int(np.floor((py + rng.uniform(-reach, reach) - g.y0) / g.dy))
            if not (0 <= iu <= g.xs - 2 and 0 <= iv <= g.ys - 2):
                continue
            t = rng.integers(1, 16) / 16.0
            x, y = g.x0 + (iu + t) * g.dx, g.y0 + (iv + t) * g.dy
        else:           # beyond a border or a corner, by 0.01 .. 0.3 m
            side, out = rng.integers(0, 8), rng.uniform(0.01, 0.3, 2)
            x, y = px + rng.uniform(-reach, reach), py + rng.uniform(-reach, reach)
            if side in (0, 4, 6): x = g.x0 - out[0]
            if side in (1, 5, 7): x = g.x1 + out[0]
            if side in (2, 4, 5): y = g.y0 - out[1]
            if side in (3, 6, 7): y = g.y1 + out[1]
            if g.inside(x, y):
                continue
        if in_reach(x, y):
            return float(x), float(y)
    return None
