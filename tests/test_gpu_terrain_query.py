"""Batched terrain height queries, height scans and ray tests on the device (rsb_get_terrain_height, rsb_height_scan, rsb_ray_test;
raisimlib_amd/csrc/rsb_terrain_query.hip) against the fp64 oracle on the float32-rounded inputs the device saw.

The test map: 9 x 7 samples (non-square: swapped axes show), 4.0 m x 3.0 m, centre (0.5, -0.25), heights uniform in +-0.2 (slopes <= 0.8), three
such maps mixed over the envs by env_map.  One oracle per map.

Bounds
  height ........ 1e-5 (1 + max |ref|) per env, normal components 1e-5: the project's bar for its fp32 queries (tests/test_gpu_parity.py).
  height scan ... 4e-5 (1 + max(|p|, |pattern|)) per env: the frames' position bar 1e-5 (1 + |p|) acts once in z and through a slope of at most
                  0.8 in x and y, plus the rounding of (c, s) times the pattern radius.
  ray test ...... a property check in fp64 with tol = 1e-5 (1 + max(|origin|, max_dist)), see check_ray.
The largest error seen per quantity goes to profiles/r10_terrain_query_parity.txt.
"""
import ctypes as C
import os

import numpy as np
import pytest

from common import ROOT, Oracle, f32, standing_states
from raisimlib_amd import BatchedWorld, _capi, workload

pytestmark = pytest.mark.gpu

XS, YS, X_SIZE, Y_SIZE, CX, CY = 9, 7, 4.0, 3.0, 0.5, -0.25
X0, Y0, DX, DY = CX - 0.5 * X_SIZE, CY - 0.5 * Y_SIZE, X_SIZE / (XS - 1), Y_SIZE / (YS - 1)
X1, Y1 = X0 + X_SIZE, Y0 + Y_SIZE
REPORT = {}


def record(section, lines):
    REPORT[section] = lines
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r10_terrain_query_parity.txt"), "w") as f:
        f.write("tests/test_gpu_terrain_query.py: largest error per quantity, device fp32 vs the fp64 oracle on the float32-rounded inputs\n")
        for name in sorted(REPORT):
            f.write(f"{name}\n" + "".join(f"  {l}\n" for l in REPORT[name]))


def make_maps(n=3, seed=11):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, (n, YS, XS)).astype(np.float32)


def map_oracles(model, maps):
    out = []
    for h in maps:
        o = Oracle(model.blob)
        o.set_heightmap(XS, YS, X_SIZE, Y_SIZE, CX, CY, h)
        out.append(o)
    return out


def map_world(model, N, maps, env_map):
    w = BatchedWorld(model, N)
    w.add_height_maps(maps, X_SIZE, Y_SIZE, CX, CY, env_map)
    return w


# ---- 1. height and normal --------------------------------------------------------------------------------------------------------------------
def height_points(N, P=130, seed=3):
    """-> xy [N, P, 2] (float32), kind [N, P]: 0 = inside a triangle, 1 = the clamped region beyond a border or a corner (both: height and
    normal), 2 = on a grid node or a diagonal (height only: the normal is discontinuous there).  Built as (cell, fx, fy)."""
    rng = np.random.default_rng(seed)
    gx, gy, kind = np.zeros((N, P)), np.zeros((N, P)), np.zeros((N, P), int)
    n_in, n_out = P // 2, 25
    for e in range(N):
        for j in range(P):
            if j < n_in:          # >= 1e-3 grid units from the cell's edges and from its diagonal, the cells and their two triangles in turn
                k = e * n_in + j
                cell, tri = k % ((XS - 1) * (YS - 1)), (k // ((XS - 1) * (YS - 1))) % 2
                lo_, hi_ = sorted(rng.uniform(2e-3, 1 - 2e-3, 2))
                if hi_ - lo_ < 3e-3:
                    lo_, hi_ = 0.25, 0.75
                fx, fy = (hi_, lo_) if tri == 0 else (lo_, hi_)
                gx[e, j], gy[e, j] = cell % (XS - 1) + fx, cell // (XS - 1) + fy
            elif j < n_in + n_out:      # beyond each border and beyond each corner; the coordinate along a border stays inside a cell's edge
                side = (j - n_in) % 8
                beyond, along = rng.uniform(1e-3, 2.0), rng.uniform(2e-3, 1 - 2e-3)
                ax, ay = rng.integers(0, XS - 1) + along, rng.integers(0, YS - 1) + along
                gx[e, j] = [-beyond, XS - 1 + beyond, ax, ax, -beyond, XS - 1 + beyond, -beyond, XS - 1 + beyond][side]
                gy[e, j] = [ay, ay, -beyond, YS - 1 + beyond, -beyond, -beyond, YS - 1 + beyond, YS - 1 + beyond][side]
                kind[e, j] = 1
            else:                 # exactly on grid nodes (the grid's coordinates are exact in float32), and on diagonals
                kind[e, j] = 2
                if j % 2:
                    gx[e, j], gy[e, j] = rng.integers(0, XS), rng.integers(0, YS)
                else:
                    f = rng.uniform(0.05, 0.95)
                    gx[e, j], gy[e, j] = rng.integers(0, XS - 1) + f, rng.integers(0, YS - 1) + f
    xy = np.stack([X0 + gx * DX, Y0 + gy * DY], axis=-1).astype(np.float32)
    return xy, kind


def test_height_and_normal_against_the_oracle(anymal):
    N, P = 8, 130
    maps = make_maps()
    env_map = np.arange(N, dtype=np.int32) % 3
    xy, kind = height_points(N, P)
    assert (kind == 0).sum() >= N * P // 2 and (kind == 1).sum() >= 8 * N and (kind == 2).sum() >= 8 * N
    w = map_world(anymal, N, maps, env_map)
    h, n = w.terrain_height(xy, normal=True)
    h_only = w.terrain_height(xy)
    assert h.shape == (N, P) and n.shape == (N, P, 3) and np.array_equal(h_only, h)
    w.close()
    oracles = map_oracles(anymal, maps)
    worst_h = worst_n = 0.0
    for e in range(N):
        ref = [oracles[env_map[e]].terrain(float(x), float(y)) for x, y in xy[e].astype(np.float64)]
        rh, rn = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        eh = float(np.abs(h[e] - rh).max() / (1.0 + np.abs(rh).max()))
        sel = kind[e] != 2
        en = float(np.abs(n[e][sel] - rn[sel]).max())
        print(f"env {e}: height {eh:.3g} normal {en:.3g}")
        worst_h, worst_n = max(worst_h, eh), max(worst_n, en)
    record("1 height and normal (N = 8, P = 130, three maps)", [f"height max |dev - ref| / (1 + max |ref|) per env = {worst_h:.3e}   (bound 1e-05)",
                                                              f"normal max |dev - ref|                       = {worst_n:.3e}   (bound 1e-05)"])
    assert worst_h <= 1e-5 and worst_n <= 1e-5, (worst_h, worst_n)


def test_ground_plane_height_is_exact(anymal):
    N, P = 3, 130
    w = BatchedWorld(anymal, N)
    w.add_ground(0.375)
    xy = np.random.default_rng(0).uniform(-50, 50, (N, P, 2)).astype(np.float32)
    h, n = w.terrain_height(xy, normal=True)
    w.close()
    assert np.all(h == np.float32(0.375)) and np.all(n == np.array([0, 0, 1], np.float32))


# ---- 2. height scan ---------------------------------------------------------------------------------------------------------------------------
def scan_pattern(nx=11, ny=3, hx=0.8, hy=0.3):
    gx, gy = np.meshgrid(np.linspace(-hx, hx, nx), np.linspace(-hy, hy, ny), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=-1).astype(np.float32)


def scan_reference(oracles, env_map, gc, frames, pattern, yaw):
    """-> ref [N, F, P] and the bound's scale max(|p|, |pattern|) per env [N], from Oracle.point_jacobian (position, rotation columns) and
    Oracle.terrain"""
    N, F, P = gc.shape[0], len(frames), pattern.shape[0]
    ref, scale = np.zeros((N, F, P)), np.zeros(N)
    pat = pattern.astype(np.float64)
    for e in range(N):
        o, q = oracles[env_map[e]], f32(gc[e])
        for k, (body, off) in enumerate(frames):
            off = f32(off)
            p, _ = o.point_jacobian(q, body, off)
            c, s = 1.0, 0.0
            if yaw:
                ex = o.point_jacobian(q, body, off + np.array([1.0, 0.0, 0.0]))[0] - p      # R e_x: (R[0], R[3], R[6])
                hy = np.hypot(ex[0], ex[1])
                assert hy > 1e-3      # (the heading is well defined in these states)
                c, s = ex[0] / hy, ex[1] / hy
            for j in range(P):
                x, y = p[0] + c * pat[j, 0] - s * pat[j, 1], p[1] + s * pat[j, 0] + c * pat[j, 1]
                ref[e, k, j] = p[2] - o.terrain(x, y)[0]
            scale[e] = max(scale[e], np.abs(p).max())
        scale[e] = max(scale[e], np.abs(pat).max())
    return ref, scale


def scan_check(dev, ref, scale, what):
    err = np.abs(dev.astype(np.float64) - ref).reshape(ref.shape[0], -1).max(axis=1) / (1.0 + scale)
    print(f"height scan {what}: max |dev - ref| / (1 + max(|p|, |pattern|)) per env = {err.max():.3g}")
    return float(err.max())


ANYMAL_SCAN_FRAMES = [("base", (0.0, 0.0, 0.0))] + [(leg + "_SHANK", (0.05, -0.02, -0.3)) for leg in ("LF", "RF", "LH", "RH")]


def test_height_scan_against_the_composition(anymal):
    N = 8
    maps = make_maps()
    env_map = (np.arange(N, dtype=np.int32) * 2) % 3
    gc, gv = standing_states(N, seed=5)      # headings over the full circle
    frames = [(anymal.body_index(b), off) for b, off in ANYMAL_SCAN_FRAMES]
    pattern = scan_pattern()
    F, P = len(frames), pattern.shape[0]
    assert P == 33
    w = map_world(anymal, N, maps, env_map)
    w.set_state(gc, gv)
    oracles = map_oracles(anymal, maps)
    lines, worst = [], 0.0
    dense = {}
    for yaw in (True, False):
        ref, scale = scan_reference(oracles, env_map, gc, frames, pattern, yaw)
        dev = w.height_scan(frames, pattern, yaw_aligned=yaw)
        assert dev.shape == (N, F, P)
        dense[yaw] = dev
        err = scan_check(dev, ref, scale, "yaw" if yaw else "world")
        lines.append(f"{'RSB_SCAN_YAW  ' if yaw else 'RSB_SCAN_WORLD'} max |dev - ref| / (1 + max(|p|, |pattern|)) per env = {err:.3e}   (bound 4e-05)")
        worst = max(worst, err)
    record("2 height scan (ANYmal-like, N = 8, base + 4 shank points, 11 x 3 pattern)", lines)
    assert worst <= 4e-5, worst
    assert not np.array_equal(dense[True], dense[False])
    # row_stride: the scan in the first F * P columns of wider rows, the other columns untouched bit for bit
    stride = F * P + 7
    for yaw in (True, False):
        buf = np.full((N, stride), -12345.678, np.float32)
        sentinel = buf[0, 0].copy()
        w.height_scan(frames, pattern, yaw_aligned=yaw, out=buf, row_stride=stride)
        assert np.array_equal(buf[:, :F * P].reshape(N, F, P), dense[yaw])
        assert np.all(buf[:, F * P:].view(np.uint32) == sentinel.view(np.uint32))
    # a frame's scan does not depend on which other frames the call lists
    a, b = frames[2], frames[0]
    both = w.height_scan([a, b], pattern)
    assert np.array_equal(both[:, 0], w.height_scan([a], pattern)[:, 0]) and np.array_equal(both[:, 1], w.height_scan([b], pattern)[:, 0])
    assert np.array_equal(both[:, 0], dense[True][:, 2]) and np.array_equal(both[:, 1], dense[True][:, 0])
    w.close()


def test_height_scan_row_stride_on_the_device(anymal):
    """torch tensors: the scan written into the tail columns of a wider observation tensor by row_stride, the head columns untouched"""
    import torch
    N, head = 8, 5
    maps = make_maps()
    env_map = np.arange(N, dtype=np.int32) % 3
    gc, gv = standing_states(N, seed=6)
    frames = [(anymal.body_index(b), off) for b, off in ANYMAL_SCAN_FRAMES]
    pattern = scan_pattern()
    F, P = len(frames), pattern.shape[0]
    w = map_world(anymal, N, maps, env_map)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    w.set_state(gc, gv)
    obs = torch.full((N, head + F * P), 7.0, dtype=torch.float32, device="cuda:0")
    w.height_scan(frames, torch.from_numpy(pattern).to("cuda:0"), out=obs[:, head:], row_stride=head + F * P)
    got = obs.cpu().numpy()
    assert np.all(got[:, :head] == 7.0)
    assert np.array_equal(got[:, head:].reshape(N, F, P), w.height_scan(frames, pattern))
    w.close()


def test_height_scan_deep_chain(atlas):
    N = 4
    maps = make_maps()
    env_map = np.array([2, 0, 1, 2], np.int32)
    gc, gv = workload.random_state(atlas.nq, atlas.nv, N, seed=4, joint_range=1.0)
    frames = [(atlas.body_index("pelvis"), (0.0, 0.0, 0.0)), (atlas.body_index("l_foot"), (0.06, 0.0, -0.05)), (atlas.body_index("r_foot"), (0.06, 0.0, -0.05))]
    pattern = scan_pattern()
    w = map_world(atlas, N, maps, env_map)
    w.set_state(gc, gv)
    oracles = map_oracles(atlas, maps)
    worst, lines = 0.0, []
    for yaw in (True, False):
        ref, scale = scan_reference(oracles, env_map, gc, frames, pattern, yaw)
        err = scan_check(w.height_scan(frames, pattern, yaw_aligned=yaw), ref, scale, "atlas yaw" if yaw else "atlas world")
        lines.append(f"{'RSB_SCAN_YAW  ' if yaw else 'RSB_SCAN_WORLD'} max |dev - ref| / (1 + max(|p|, |pattern|)) per env = {err:.3e}   (bound 4e-05)")
        worst = max(worst, err)
    w.close()
    record("2b height scan (Atlas-like, N = 4, pelvis + both feet)", lines)
    assert worst <= 4e-5, worst


# ---- 3. ray test ------------------------------------------------------------------------------------------------------------------------------
def ray_inputs(N=6, R=150, hmax=0.2, seed=8):
    rng = np.random.default_rng(seed)
    o, d = np.zeros((N, R, 3)), np.zeros((N, R, 3))
    for e in range(N):
        for r in range(R):
            if r % 4 != 3:      # inside the footprint, at least 0.2 above the highest sample
                o[e, r] = [rng.uniform(X0, X1), rng.uniform(Y0, Y1), hmax + rng.uniform(0.2, 1.2)]
            else:               # up to 1 m outside it, at the terrain's own heights and above
                side = rng.integers(0, 4)
                out, along_x, along_y = rng.uniform(0.01, 1.0), rng.uniform(X0 - 1, X1 + 1), rng.uniform(Y0 - 1, Y1 + 1)
                o[e, r, :2] = [(X0 - out, along_y), (X1 + out, along_y), (along_x, Y0 - out), (along_x, Y1 + out)][side]
                o[e, r, 2] = rng.uniform(-0.3, 0.8)
            kind = (r // 4 + r + e) % 8
            ang = rng.uniform(0, 2 * np.pi)
            if kind == 0: v = np.array([0.0, 0.0, -1.0])
            elif kind == 1: v = np.array([1.0, 0.0, -0.2])
            elif kind == 2: v = np.array([0.0, -1.0, -0.3])
            elif kind == 3: v = np.array([1.0, 1.0, -0.25])
            elif kind == 4: v = np.array([np.cos(ang), np.sin(ang), rng.uniform(0.02, 1.0)])               # upward
            elif kind == 5: v = np.array([np.cos(ang), np.sin(ang), -rng.uniform(0.05, 0.5)])              # shallow
            elif kind == 6: v = np.array([0.3 * rng.uniform() * np.cos(ang), 0.3 * rng.uniform() * np.sin(ang), -1.0])   # steep
            else:
                v = rng.normal(size=3); v[2] = -abs(v[2])                                                      # lower hemisphere
            d[e, r] = v * rng.uniform(0.5, 3.0)
    return o.astype(np.float32), d.astype(np.float32)


def ray_breakpoints(o, d, max_dist):
    """fp64: (lo, hi, sorted parameters in [lo, hi] where z - h may bend, unit direction) of one ray against the footprint, or None if the ray
    never meets it.  u = (x - x0) / dx, v = (y - y0) / dy: breakpoints where u, v or u - v is an integer, plus lo and hi."""
    dn = d / np.linalg.norm(d)
    lo, hi = 0.0, float(max_dist)
    for a, b, p, q in ((X0, X1, o[0], dn[0]), (Y0, Y1, o[1], dn[1])):
        if q == 0.0:
            if p < a or p > b:
                return None
        else:
            s0, s1 = sorted(((a - p) / q, (b - p) / q))
            lo, hi = max(lo, s0), min(hi, s1)
    if lo > hi:
        return None
    u0, v0, du, dv = (o[0] - X0) / DX, (o[1] - Y0) / DY, dn[0] / DX, dn[1] / DY
    s = [lo, hi]
    if du != 0.0: s += [(i - u0) / du for i in range(XS)]
    if dv != 0.0: s += [(i - v0) / dv for i in range(YS)]
    if du != dv: s += [(k - (u0 - v0)) / (du - dv) for k in range(-(YS - 1), XS)]
    s = np.array(sorted(x for x in s if lo <= x <= hi))
    return lo, hi, s, dn


def gap(oracle, o, dn, s):
    return o[2] + s * dn[2] - oracle.terrain(o[0] + s * dn[0], o[1] + s * dn[1])[0]


def ray_reference(oracle, o, d, max_dist):
    """-> (distance or -1, is a wall hit) of the fp64 reference alone"""
    bp = ray_breakpoints(o, d, max_dist)
    if bp is None:
        return -1.0, False
    lo, hi, s, dn = bp
    g = np.array([gap(oracle, o, dn, x) for x in s])
    below = np.nonzero(g <= 0.0)[0]
    if below.size == 0:
        return -1.0, False
    k = below[0]
    if k == 0:
        return lo, lo > 0.0
    return s[k - 1] + (s[k] - s[k - 1]) * g[k - 1] / (g[k - 1] - g[k]), False


def check_ray(oracle, o, d, max_dist, t):
    """the property check of one device result t -> (ok, residual / tol, what failed); z - h is piecewise linear with bends at the
    breakpoints only, so looking at the breakpoints, lo, hi and t is exact"""
    tol = 1e-5 * (1.0 + max(np.abs(o).max(), max_dist))
    bp = ray_breakpoints(o, d, max_dist)
    if bp is None:
        return (t == -1.0), 0.0, "a ray that never meets the footprint must miss"
    lo, hi, s, dn = bp
    g = np.array([gap(oracle, o, dn, x) for x in s])
    if t == -1.0:
        worst = float(max(0.0, -g.min()))
        return worst <= tol, worst / tol, "a miss, but the ray is below the surface at a breakpoint"
    gt = gap(oracle, o, dn, t)
    before = g[s < t - tol]
    res = max(lo - t, t - hi, gt, float(-before.min()) if before.size else 0.0, 0.0 if t <= lo + tol else -gt)
    if not (lo - tol <= t <= hi + tol):
        return False, res / tol, "the hit is outside [lo, hi]"
    if not gt <= tol:
        return False, res / tol, "the hit is above the surface"
    if before.size and not before.min() >= -tol:
        return False, res / tol, "the ray is below the surface before the hit"
    if not (gt >= -tol or t <= lo + tol):
        return False, res / tol, "the hit is below the surface and not at the wall"
    return True, max(res, 0.0) / tol, ""


def test_ray_test_properties_in_fp64(anymal):
    N, R, max_dist = 6, 150, 6.0
    maps = make_maps()
    env_map = np.arange(N, dtype=np.int32) % 3
    o32, d32 = ray_inputs(N, R, hmax=float(maps.max()))
    oracles = map_oracles(anymal, maps)
    o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
    # the inputs, on the reference alone: enough hits, enough misses, a wall hit
    ref = [[ray_reference(oracles[env_map[e]], o64[e, r], d64[e, r], max_dist) for r in range(R)] for e in range(N)]
    hits = sum(t >= 0 for row in ref for t, _ in row)
    walls = sum(wall for row in ref for _, wall in row)
    print(f"reference: {hits} hits of {N * R}, {walls} wall hits")
    assert hits >= 0.15 * N * R and N * R - hits >= 0.15 * N * R and walls >= 1
    w = map_world(anymal, N, maps, env_map)
    t = w.ray_test(o32, d32, max_dist)
    w.close()
    assert t.shape == (N, R)
    bad, worst = [], 0.0
    for e in range(N):
        for r in range(R):
            ok, res, why = check_ray(oracles[env_map[e]], o64[e, r], d64[e, r], max_dist, float(t[e, r]))
            worst = max(worst, res)
            if not ok:
                bad.append((e, r, float(t[e, r]), ref[e][r][0], why))
    dev_hits = int((t >= 0).sum())
    print(f"device: {dev_hits} hits, worst residual {worst:.3g} tol, {len(bad)} violations {bad[:5]}")
    record("3 ray test (N = 6, R = 150, max_dist = 6, three maps)", [f"{dev_hits} hits of {N * R} rays ({hits} in the fp64 reference, {walls} wall hits)",
                                                                    f"worst residual of the property check = {worst:.3e} tol, {len(bad)} violations"])
    assert not bad, bad[:10]


def test_ray_test_known_answers(anymal):
    rng = np.random.default_rng(2)
    N, R, max_dist = 2, 64, 6.0
    tol = lambda o: 1e-5 * (1.0 + max(float(np.nanmax(np.abs(o))), max_dist))      # noqa: E731
    # the ground plane z = z0 in closed form; ray 0 parallel to it and ray 1 pointing up miss; NaN / zero rays give -1
    z0 = 0.25
    o = np.stack([rng.uniform(-3, 3, (N, R)), rng.uniform(-3, 3, (N, R)), z0 + rng.uniform(0.1, 2.0, (N, R))], axis=-1).astype(np.float32)
    d = rng.normal(size=(N, R, 3)).astype(np.float32)
    d[:, 0] = [1.0, 2.0, 0.0]
    d[:, 1] = [0.3, -0.2, 0.5]
    d[:, 2] = [0.0, 0.0, -2.5]
    o[:, 3, 2] = z0 - 0.5      # an origin below the plane
    d[0, 4], d[0, 5], o[0, 6, 1] = [np.nan, 0.0, -1.0], [0.0, 0.0, 0.0], np.nan
    w = BatchedWorld(anymal, N)
    w.add_ground(z0)
    t = w.ray_test(o, d, max_dist)      # (RSB_OK: check() raises otherwise)
    w.close()
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    dn = d64 / np.linalg.norm(d64, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (z0 - o64[..., 2]) / dn[..., 2]
    want = np.where((dn[..., 2] < 0) & (s <= max_dist), s, -1.0)
    want[:, 3] = 0.0
    want[0, 4:7] = -1.0
    assert np.all(t[:, 0] == -1) and np.all(t[:, 1] == -1) and np.all(t[0, 4:7] == -1) and np.all(t[:, 3] == 0)
    assert np.all((t == -1) == (want == -1)), np.nonzero((t == -1) != (want == -1))
    assert np.all(np.abs(t - want) <= np.array([[tol(o[e, r]) for r in range(R)] for e in range(N)]))
    assert abs(t[1, 2] - (o64[1, 2, 2] - z0)) <= tol(o[1, 2])
    # a constant map equals the plane inside the footprint; a ramp h = a x in closed form; degenerate rays on a map
    a = 0.3
    flat = np.full((1, YS, XS), z0, np.float32)
    ramp = (a * (X0 + DX * np.arange(XS)))[None, None, :].repeat(YS, axis=1).astype(np.float32)
    o = np.stack([rng.uniform(X0 + 0.2, X1 - 0.2, (N, R)), rng.uniform(Y0 + 0.2, Y1 - 0.2, (N, R)), 1.2 + rng.uniform(0.0, 1.0, (N, R))], axis=-1).astype(np.float32)
    d = np.stack([rng.normal(size=(N, R)) * 0.3, rng.normal(size=(N, R)) * 0.3, -rng.uniform(0.5, 2.0, (N, R))], axis=-1).astype(np.float32)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    dn = d64 / np.linalg.norm(d64, axis=-1, keepdims=True)
    for maps, s in ((flat, (z0 - o64[..., 2]) / dn[..., 2]), (ramp, (a * o64[..., 0] - o64[..., 2]) / (dn[..., 2] - a * dn[..., 0]))):
        w = map_world(anymal, N, maps, np.zeros(N, np.int32))
        hit_xy = o64[..., :2] + s[..., None] * dn[..., :2]
        inside = (hit_xy[..., 0] > X0) & (hit_xy[..., 0] < X1) & (hit_xy[..., 1] > Y0) & (hit_xy[..., 1] < Y1) & (s <= max_dist)
        assert inside.sum() > N * R // 2
        t = w.ray_test(o, d, max_dist)
        err = np.abs(t - s)[inside]
        print(f"closed form: max |t - s| = {err.max():.3g}")
        assert np.all(err <= np.array([[tol(o[e, r]) for r in range(R)] for e in range(N)])[inside])
        assert np.all(t[~inside] == -1)      # they leave the footprint above the surface
        dd, oo = d.copy(), o.copy()
        dd[0, 0], dd[0, 1], oo[0, 2, 0] = [0.0, np.nan, -1.0], [0.0, 0.0, 0.0], np.nan
        t2 = w.ray_test(oo, dd, max_dist)
        assert np.all(t2[0, :3] == -1) and np.array_equal(t2[0, 3:], t[0, 3:]) and np.array_equal(t2[1], t[1])
        w.close()


# ---- 4. stream order and device pointers ---------------------------------------------------------------------------------------------------------
def test_device_pointers_follow_the_stream(anymal):
    """torch CUDA tensors in and out, right after integrate and after set_state with no synchronisation between: the bits of the RSB_HOST form,
    and the scan follows the new state"""
    import torch
    N = 8
    maps = make_maps()
    env_map = np.arange(N, dtype=np.int32) % 3
    gc, gv = standing_states(N, seed=7)
    frames = [(anymal.body_index(b), off) for b, off in ANYMAL_SCAN_FRAMES]
    pattern = scan_pattern()
    F, P = len(frames), pattern.shape[0]
    xy, _ = height_points(N)
    o32, d32 = ray_inputs(N, 40, hmax=float(maps.max()))
    dev = torch.device("cuda:0")
    w = map_world(anymal, N, maps, env_map)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    w.set_state(gc, gv)
    txy, tpat, to, td = (torch.from_numpy(a).to(dev) for a in (xy, pattern, o32, d32))
    scans = []
    for change in ("integrate", "set_state"):
        th = torch.full((N, xy.shape[1]), 7.0, dtype=torch.float32, device=dev)
        tn = torch.full((N, xy.shape[1], 3), 7.0, dtype=torch.float32, device=dev)
        ts = torch.full((N, F, P), 7.0, dtype=torch.float32, device=dev)
        tt = torch.full((N, 40), 7.0, dtype=torch.float32, device=dev)
        if change == "integrate":
            w.integrate(4)
        else:
            w.set_state(gc[::-1].copy(), gv[::-1].copy())
        w.terrain_height(txy, out={"height": th, "normal": tn})
        assert w.height_scan(frames, tpat, out=ts) is ts
        w.ray_test(to, td, 6.0, out=tt)
        h, n = w.terrain_height(xy, normal=True)
        assert np.array_equal(th.cpu().numpy(), h) and np.array_equal(tn.cpu().numpy(), n)
        assert np.array_equal(ts.cpu().numpy(), w.height_scan(frames, pattern))
        assert np.array_equal(tt.cpu().numpy(), w.ray_test(o32, d32, 6.0))
        scans.append(ts.cpu().numpy())
    # the scan of the state set last, from a world that never saw another one
    w2 = map_world(anymal, N, maps, env_map)
    w2.set_state(gc[::-1].copy(), gv[::-1].copy())
    assert np.array_equal(scans[1], w2.height_scan(frames, pattern)) and not np.array_equal(scans[0], scans[1])
    w2.close()
    w.close()


# ---- 5. arguments -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(anymal, built_lib):
    L = built_lib
    N = 2
    w = BatchedWorld(anymal, N)
    w.add_ground(0.0)
    buf = np.zeros(N * 4096 * 3, np.float32)
    out = np.full(N * 4096, 5.0, np.float32)
    p, q = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 2)()
    bad = (_capi.Frame * 1)()
    bad[0].body = anymal.nb
    H = w.handle
    cases = [
        lambda: L.rsb_get_terrain_height(None, p, 4, q, None, 0),
        lambda: L.rsb_get_terrain_height(H, p, 4, None, None, 0),
        lambda: L.rsb_get_terrain_height(H, p, 0, q, None, 0),
        lambda: L.rsb_height_scan(None, fr, 1, p, 4, 1, q, 0, 0),
        lambda: L.rsb_height_scan(H, fr, 1, p, 4, 1, None, 0, 0),
        lambda: L.rsb_height_scan(H, fr, 1, p, 0, 1, q, 0, 0),
        lambda: L.rsb_height_scan(H, fr, 1, p, _capi.RSB_MAX_SCAN_POINTS + 1, 1, q, 0, 0),
        lambda: L.rsb_height_scan(H, bad, 1, p, 4, 1, q, 0, 0),
        lambda: L.rsb_height_scan(H, fr, 1, p, 4, 2, q, 0, 0),
        lambda: L.rsb_height_scan(H, fr, 2, p, 4, 1, q, 7, 0),
        lambda: L.rsb_height_scan(H, fr, 2, p, 4, 1, q, -1, 0),
        lambda: L.rsb_ray_test(None, p, p, 4, 1.0, q, 0),
        lambda: L.rsb_ray_test(H, p, p, 4, 1.0, None, 0),
        lambda: L.rsb_ray_test(H, p, p, 0, 1.0, q, 0),
        lambda: L.rsb_ray_test(H, p, p, 4, 0.0, q, 0),
        lambda: L.rsb_ray_test(H, p, p, 4, -1.0, q, 0),
        lambda: L.rsb_ray_test(H, p, p, 4, float("inf"), q, 0),
        lambda: L.rsb_ray_test(H, p, p, 4, float("nan"), q, 0),
    ]
    for k, call in enumerate(cases):
        assert call() == -1, k      # RSB_E_INVALID
        assert len(L.rsb_last_error()) > 10, k
    assert np.all(out == 5.0)      # nothing was launched
    # the limits themselves are accepted
    pat = np.zeros((_capi.RSB_MAX_SCAN_POINTS, 2), np.float32)
    assert w.height_scan([0], pat).shape == (N, 1, _capi.RSB_MAX_SCAN_POINTS)
    w.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_against_the_host_height_map(built_lib):
    """BatchedWorld::getTerrainHeights / heightScan / rayTest (tests/cpp/terrain_query_facade_test.cpp) against HeightMap::getHeight in double"""
    import subprocess
    from test_terrain_query_host import BIN, URDF, compile_terrain_query_facade
    compile_terrain_query_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "terrain_query_facade_test OK" in r.stdout
