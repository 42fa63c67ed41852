"""The fp64 reference of the ray casts that also hit the robot (rsb_ray_cast, rsb_ray_scan; include/rsb.h), in numpy.  It shares nothing with the
kernels: the shapes are read from the model blob by the rules of rsb.h, their exact signed distances phi are written from the definitions, the
entry and exit parameters of a ray are closed forms in fp64, and a device answer is judged by a PROPERTY check on phi, not by comparing ranges.

The property check (check_answer), with tol = 1e-5 (1 + max(|origin|, max_dist)) - the bar check_ray of tests/test_gpu_terrain_query.py sets for
the terrain.  phi_union = the smallest phi over the shapes the ray may see; it is looked at along the ray at the reference's entry, exit and
closest-approach parameters of every shape the line goes through (past a convex shape it misses phi stays positive: such a shape can put no
sample inside anything) and at 1000 evenly spaced parameters of [0, max_dist].
  a body hit at t ...... |phi_union(x(t))| <= tol, or t <= tol and phi_union <= tol (an origin inside a shape); no sample before t - tol has
                         phi_union < -tol; `hit` names a shape with phi(x(t)) <= tol whose body the own-body rule allows; the terrain is not
                         deeper than tol under any of its own breakpoints before t - tol.
  a terrain hit at t ... the terrain's own check passes; no sample before t - tol is deeper than tol in a shape.
  a miss ............... no sample of [0, max_dist] is deeper than tol in a shape; the terrain's miss condition holds.
At grazing incidence phi moves little for a large change of t: a hit and a miss both pass there, so no ray is excluded and no cap is needed.
Returned with the verdict: the largest residual in units of tol.
"""
import numpy as np

HIT_NONE, HIT_TERRAIN = -1, -2
SAMPLES = 1000


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------------
def shapes_of(blob):
    """the robot as rays see it -> [dict(kind, body, prim, ...)] in the body frame.  The collision primitives in index order:
      col_capsule[s] == -1                     box: centre = mean of the corners s .. s + 7, half-edges (c[s+1] - c[s]) / 2, (c[s+2] - c[s]) / 2, (c[s+4] - c[s]) / 2
      col_capsule[s] = e + 1, col_rim[s] == 0  capsule: segment col_pos[s] - col_pos[e], radius col_radius[s]
      col_capsule[s] = e + 1, col_rim[s] > 0   cylinder with flat caps: axis col_pos[s] - col_pos[e], radius col_rim[s]
      another primitive with col_radius > 0    sphere
    everything else (zero-radius points) has no surface.  (A box with an edge of zero length has no volume and is left out.)"""
    pos = np.array([[blob.col_pos[s][k] for k in range(3)] for s in range(blob.ncol)], np.float64).reshape(-1, 3)
    used, out = set(), []
    for s in range(blob.ncol):
        if s in used:
            continue
        cap, body = int(blob.col_capsule[s]), int(blob.col_body[s])
        if cap == -1:
            used.update(range(s, s + 8))
            half = np.stack([(pos[s + 1] - pos[s]) / 2, (pos[s + 2] - pos[s]) / 2, (pos[s + 4] - pos[s]) / 2])
            if np.all(np.linalg.norm(half, axis=1) > 0):
                out.append(dict(kind="box", body=body, prim=s, centre=pos[s:s + 8].mean(axis=0), half=half))
        elif cap > 0:
            e = cap - 1
            used.add(e)
            if blob.col_rim[s] > 0:
                out.append(dict(kind="cylinder", body=body, prim=s, a=pos[s], b=pos[e], radius=float(blob.col_rim[s])))
            else:
                out.append(dict(kind="capsule", body=body, prim=s, a=pos[s], b=pos[e], radius=float(blob.col_radius[s])))
        elif blob.col_radius[s] > 0:
            out.append(dict(kind="sphere", body=body, prim=s, centre=pos[s], radius=float(blob.col_radius[s])))
    return out


def body_poses(oracle, q):
    """(R [3,3], p [3]) of every body at the configuration q (fp64), from Oracle.point_jacobian alone, as tests/test_gpu_frames.py takes them"""
    out = []
    for b in range(oracle.nb):
        p = oracle.point_jacobian(q, b, np.zeros(3))[0]
        R = np.stack([oracle.point_jacobian(q, b, np.eye(3)[k])[0] - p for k in range(3)], axis=1)
        out.append((R, p))
    return out


def to_world(shape, poses):
    R, p = poses[shape["body"]]
    w = dict(shape)
    for k in ("centre", "a", "b"):
        if k in shape:
            w[k] = p + R @ shape[k]
    if "half" in shape:
        w["half"] = shape["half"] @ R.T
    return w


# ---- exact signed distances ----------------------------------------------------------------------------------------------------------------------
def phi(shape, x):
    """signed distance of the points x [..., 3] to the surface of a shape, negative inside"""
    x = np.asarray(x, np.float64)
    kind = shape["kind"]
    if kind == "sphere":
        return np.linalg.norm(x - shape["centre"], axis=-1) - shape["radius"]
    if kind == "box":
        h = np.linalg.norm(shape["half"], axis=1)
        u = shape["half"] / h[:, None]
        q = np.abs((x - shape["centre"]) @ u.T) - h
        return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    a, b, r = shape["a"], shape["b"], shape["radius"]
    L = np.linalg.norm(b - a)
    n = (b - a) / L if L > 0 else np.array([0.0, 0.0, 1.0])
    m = x - a
    y = m @ n
    if kind == "capsule":
        yc = np.clip(y, 0.0, L)
        return np.linalg.norm(m - yc[..., None] * n, axis=-1) - r
    rad = np.linalg.norm(m - y[..., None] * n, axis=-1)      # cylinder: the rectangle (radial, axial) in two dimensions
    dr, da = rad - r, np.abs(y - 0.5 * L) - 0.5 * L
    return np.hypot(np.maximum(dr, 0.0), np.maximum(da, 0.0)) + np.minimum(np.maximum(dr, da), 0.0)


# ---- a ray against a shape, closed forms -----------------------------------------------------------------------------------------------------------
def _ball(c, r, o, d):
    m = o - c
    b, cc = m @ d, m @ m - r * r
    disc = b * b - cc
    if disc < 0:
        return None
    return -b - np.sqrt(disc), -b + np.sqrt(disc)


def _tube(a, n, L, r, o, d):
    """the infinite cylinder about the axis through a along n, cut by the slab 0 <= (x - a) . n <= L"""
    m = o - a
    mn, dn = m @ n, d @ n
    mp, dp = m - mn * n, d - dn * n
    A, B, Cc = dp @ dp, mp @ dp, mp @ mp - r * r
    if A < 1e-300:
        if Cc > 0:
            return None
        t0, t1 = -np.inf, np.inf
    else:
        disc = B * B - A * Cc
        if disc < 0:
            return None
        t0, t1 = (-B - np.sqrt(disc)) / A, (-B + np.sqrt(disc)) / A
    if dn == 0.0:
        if mn < 0 or mn > L:
            return None
    else:
        s0, s1 = sorted((-mn / dn, (L - mn) / dn))
        t0, t1 = max(t0, s0), min(t1, s1)
    return (t0, t1) if t0 <= t1 else None


def interval(shape, o, d):
    """(t_in, t_out) of the whole line o + t d (d a unit vector) through a shape, or None if it passes by.  Every shape is convex: one interval."""
    kind = shape["kind"]
    if kind == "sphere":
        return _ball(shape["centre"], shape["radius"], o, d)
    if kind == "box":
        h2 = (shape["half"] ** 2).sum(axis=1)
        oi, di = (shape["half"] @ (o - shape["centre"])) / h2, (shape["half"] @ d) / h2
        t0, t1 = -np.inf, np.inf
        for k in range(3):
            if di[k] == 0.0:
                if abs(oi[k]) > 1.0:
                    return None
            else:
                s0, s1 = sorted(((-1.0 - oi[k]) / di[k], (1.0 - oi[k]) / di[k]))
                t0, t1 = max(t0, s0), min(t1, s1)
        return (t0, t1) if t0 <= t1 else None
    a, b, r = shape["a"], shape["b"], shape["radius"]
    L = np.linalg.norm(b - a)
    n = (b - a) / L if L > 0 else np.array([0.0, 0.0, 1.0])
    parts = [_tube(a, n, L, r, o, d)] if L > 0 else []
    if kind == "capsule":
        parts += [_ball(a, r, o, d), _ball(b, r, o, d)]
    parts = [p for p in parts if p is not None]
    if not parts:
        return None
    return min(p[0] for p in parts), max(p[1] for p in parts)      # (the parts of a capsule overlap: their union is one interval)


def first_entry(shape, o, d, max_dist):
    """the first parameter of [0, max_dist] at which the ray is on or inside the shape, or None"""
    iv = interval(shape, o, d)
    if iv is None or iv[1] < 0.0 or iv[0] > max_dist:
        return None
    return max(iv[0], 0.0)


def closest_parameter(shape, o, d, lo, hi):
    """the parameter of [lo, hi] where the ray is deepest in the shape: phi along a ray is convex, so a golden-section search"""
    g = 0.5 * (np.sqrt(5.0) - 1.0)
    f = lambda t: float(phi(shape, o + t * d))      # noqa: E731
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(40):
        if f1 <= f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo)
            f1 = f(x1)
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo)
            f2 = f(x2)
    return 0.5 * (lo + hi)


def reference_cast(shapes, allowed, o, d, max_dist):
    """(range, prim) of the first body entry among the allowed world-frame shapes, or (-1, HIT_NONE): the reference's own answer (for choosing test
    inputs; the device is judged by check_answer)"""
    dn = d / np.linalg.norm(d)
    best, prim = np.inf, HIT_NONE
    for s, ok in zip(shapes, allowed):
        t = first_entry(s, o, dn, max_dist) if ok else None
        if t is not None and t < best:
            best, prim = t, s["prim"]
    return (best, prim) if prim != HIT_NONE else (-1.0, HIT_NONE)


# ---- the terrain's side of the check --------------------------------------------------------------------------------------------------------------
class PlaneTerrain:
    """the infinite plane z = z0 (a height map's counterpart wraps check_ray: tests/test_gpu_ray_scan.py)"""

    def __init__(self, z0):
        self.z0 = float(z0)

    def deepest_before(self, o, dn, max_dist, t_end):
        """how far below the surface the ray gets on [0, t_end]"""
        if t_end <= 0.0:
            return 0.0
        return max(0.0, self.z0 - o[2], self.z0 - (o[2] + t_end * dn[2]))

    def check(self, o, d, max_dist, t):
        """(ok, residual / tol, why) of the terrain answer t (-1: a miss)"""
        tol = 1e-5 * (1.0 + max(np.abs(o).max(), max_dist))
        dn = d / np.linalg.norm(d)
        if t == -1.0:
            worst = self.deepest_before(o, dn, max_dist, max_dist)
            return worst <= tol, worst / tol, "a miss, but the ray gets below the plane"
        g = o[2] + t * dn[2] - self.z0
        res = max(-t, t - max_dist, g, self.deepest_before(o, dn, max_dist, t - tol), 0.0 if t <= tol else -g)
        return res <= tol, max(res, 0.0) / tol, "the plane hit is off the plane, outside [0, max_dist] or behind a crossing"


# ---- the property check ---------------------------------------------------------------------------------------------------------------------------
def check_answer(shapes, allowed, o, d, max_dist, t, hit, terrain):
    """One device answer (t, hit) for the ray (o, d) against the world-frame shapes (allowed[k]: the own-body rule lets the ray see shape k) and
    the terrain (an object with check and deepest_before) -> (ok, worst residual / tol, why)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tol = 1e-5 * (1.0 + max(np.abs(o).max(), max_dist))
    dn = d / np.linalg.norm(d)
    live = [s for s, ok in zip(shapes, allowed) if ok]
    # a line that passes a (convex) shape by has phi > 0 all along: only the shapes it goes through can put a sample inside a shape
    params, crossed = [np.linspace(0.0, max_dist, SAMPLES)], []
    for s in live:
        iv = interval(s, o, dn)
        if iv is None or iv[1] < 0.0 or iv[0] > max_dist:
            continue
        crossed.append(s)
        lo, hi = max(iv[0], 0.0), min(iv[1], max_dist)
        params.append(np.array([iv[0], iv[1], closest_parameter(s, o, dn, lo, hi)]))
    P = np.concatenate(params)
    P = np.sort(P[(P >= 0.0) & (P <= max_dist)])
    X = o + P[:, None] * dn
    union = np.min([phi(s, X) for s in crossed], axis=0) if crossed else np.full(P.shape, np.inf)
    if hit == HIT_NONE:
        if t != -1.0:
            return False, np.inf, "a miss must report -1"
        deepest = float(max(0.0, -union.min()))
        ok_t, res_t, why_t = terrain.check(o, d, max_dist, -1.0)
        if deepest > tol:
            return False, deepest / tol, "a miss, but the ray is inside a shape"
        return ok_t, max(res_t, deepest / tol), why_t
    if not (0.0 <= t <= max_dist + tol):
        return False, np.inf, "the hit is outside [0, max_dist]"
    before = union[P < t - tol]
    deepest = float(max(0.0, -before.min())) if before.size else 0.0
    if deepest > tol:
        return False, deepest / tol, "the ray is inside a shape before the hit"
    if hit == HIT_TERRAIN:
        ok_t, res_t, why_t = terrain.check(o, d, max_dist, t)
        return ok_t, max(res_t, deepest / tol), why_t
    xt = o + t * dn
    phis = np.array([float(phi(s, xt)) for s in live]) if live else np.array([np.inf])
    u = float(phis.min())
    res = max(deepest, u if t <= tol else abs(u))
    if res > tol:
        return False, res / tol, "the body hit is not on a surface (nor an origin inside a shape)"
    named = [k for k, s in enumerate(live) if s["prim"] == hit]
    if not named:
        return False, np.inf, "hit names no shape the ray may see"
    res = max(res, float(phis[named[0]]))
    if phis[named[0]] > tol:
        return False, res / tol, "hit names a shape the ray is not on"
    under = terrain.deepest_before(o, dn, max_dist, t - tol)
    res = max(res, under)
    return under <= tol, res / tol, "the terrain is crossed before the body hit"
