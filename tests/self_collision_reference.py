"""Independent statement of self-collision (numpy, fp64): what rsb.h and the step kernel's comments SAY the candidate list, the sphere x sphere narrow
phase and the contact-list assembly are, written as a brute force - not a third copy of enumerate_self_pairs / self_pair_ok and of the kernel's rare
path.  Imports nothing from oracle/; of what the library computes it reads only the model blob's static tables (parent, col_body, col_pos, col_radius,
col_rim, joint origins, axes and types).  Used by tests/test_self_collision_reference.py (pins the oracle) and tests/test_gpu_self_collision.py (the device).

Kinematics   tree of a floating or fixed base, revolute and prismatic joints, joint origins with xyz only: body b has R_b = R_parent Rodrigues(axis_b, q_b)
             (revolute) or R_parent (prismatic), p_b = p_parent + R_parent (origin_b [+ axis_b q_b, prismatic]); a primitive's centre is p_b + R_b col_pos.
             State as in rsb_set_state: q = (p, quaternion w x y z, joints in body order); evaluated on the float32-rounded state, in fp64.
Candidates   primitive pairs i < j, i-major, of two different bodies that are not parent and child; neither is a rim primitive; r_i + r_j > 0; the
             body pair is not in the caller's (symmetric) ignore set.
Narrow phase every candidate pair: hit iff |c_i - c_j| < r_i + r_j and |c_i - c_j|^2 >= 1e-12; depth r_i + r_j - dist; normal from j to i;
             point c_i - (r_i - depth / 2) n.
List         terrain contacts first (taken as given), then per hit, in pair order, (i | SELF_A, body_i) and (j | SELF_B, body_j): the B entry has the opposite
             normal, the same position and - in the reported list, rsb_types.h - the same depth (inside the solver its slot carries depth 0: the fold adds the two).  A hit that would not get both of the kmax slots is dropped with every later one, overflow flag bit 0.  Joint-limit
             rows then take slots while any remain (the odd one included); they are not reported, a row without a slot sets flag bit 0.
Closed forms head_on() and tangential() at the end: two sliders meeting under Newton restitution with a threshold and Coulomb friction.

Designed models ("combs", class Comb): everything lies in the plane z = 0 of the base.  Limb k slides along a line (prismatic, axis a_k through o_k) and carries
spheres ON that line; its elbow turns about z around a hinge on the line and carries spheres at radius rho, so an elbow sphere reaches every point within rho
of its line.  Two limb spheres meet where their lines cross, an elbow sphere meets anything inside its band, the base's spheres sit inside the bands of two
lines.  Each placement is found in closed form, polished by a secant step on one coordinate to the wanted centre distance, and ACCEPTED ONLY after the
brute force above confirms the wanted hit set with every other pair at least `clear` apart; rejected tries are repeated with other random choices."""
import numpy as np

SELF_A, SELF_B = 0x10000, 0x20000
REVOLUTE, PRISMATIC = 1, 2
COINCIDENT2 = 1e-12


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


class Tables:
    """the static tables of a model blob this reference is allowed to read"""

    def __init__(self, blob):
        nb, nc = blob.nb, blob.ncol
        self.nb, self.ncol = nb, nc
        self.parent = np.array([blob.parent[b] for b in range(nb)])
        self.jtype = np.array([blob.jtype[b] for b in range(nb)])
        self.axis = np.array([list(blob.axis[b]) for b in range(nb)])
        self.origin = np.array([list(blob.ptree[b]) for b in range(nb)])
        self.col_body = np.array([blob.col_body[s] for s in range(nc)])
        self.col_pos = np.array([list(blob.col_pos[s]) for s in range(nc)])
        self.col_radius = np.array([blob.col_radius[s] for s in range(nc)])
        self.col_rim = np.array([blob.col_rim[s] for s in range(nc)])
        # what the device holds of the primitives: float32
        self.pos32, self.rad32 = f32(self.col_pos), f32(self.col_radius)


def body_frames(T, q):
    q = np.asarray(q, np.float64)
    R, p = [None] * T.nb, [None] * T.nb
    R[0], p[0] = quat_to_rot(q[3:7] / np.linalg.norm(q[3:7])), q[:3].copy()
    for b in range(1, T.nb):      # (bodies are numbered parents first)
        pa, qb = T.parent[b], q[6 + b]
        assert pa < b
        if T.jtype[b] == REVOLUTE:
            R[b], p[b] = R[pa] @ rodrigues(T.axis[b], qb), p[pa] + R[pa] @ T.origin[b]
        else:
            assert T.jtype[b] == PRISMATIC
            R[b], p[b] = R[pa], p[pa] + R[pa] @ (T.origin[b] + T.axis[b] / np.linalg.norm(T.axis[b]) * qb)
    return R, p


def centres(T, q, single=False):
    """world centres [ncol, 3]; single: the primitive offsets as the device holds them (float32)"""
    R, p = body_frames(T, q)
    off = T.pos32 if single else T.col_pos
    return np.array([p[T.col_body[s]] + R[T.col_body[s]] @ off[s] for s in range(T.ncol)])


def candidate_pairs(T, ignore=()):
    """[(i, j)] in i-major order; ignore: body pairs, either order"""
    ign = {frozenset(bp) for bp in ignore}
    out = []
    for i in range(T.ncol):
        for j in range(i + 1, T.ncol):
            a, b = T.col_body[i], T.col_body[j]
            if a == b or T.parent[a] == b or T.parent[b] == a or frozenset((a, b)) in ign:
                continue
            if T.col_rim[i] > 0 or T.col_rim[j] > 0 or not T.col_radius[i] + T.col_radius[j] > 0:
                continue
            out.append((i, j))
    return np.array(out, np.int64).reshape(-1, 2)


def pair_distances(T, pairs, c, single=False):
    rad = T.rad32 if single else T.col_radius
    d = np.linalg.norm(c[pairs[:, 0]] - c[pairs[:, 1]], axis=1) if len(pairs) else np.zeros(0)
    return d, (rad[pairs[:, 0]] + rad[pairs[:, 1]] if len(pairs) else np.zeros(0))


def limit_rows(q, limits):
    """number of joints outside their range; limits: {body: (lower, upper)}"""
    return sum(1 for b, (lo, hi) in limits.items() if lo < hi and not lo <= float(q[6 + b]) <= hi)


def assemble(n0, hits, n_lim, kmax):
    """-> (hits kept, reported count, overflow flag, limit rows that got a slot)"""
    kept, used, over = [], n0, False
    for h in hits:
        if over or used + 2 > kmax:
            over = True
            continue
        kept.append(h)
        used += 2
    rows = min(n_lim, kmax - used)
    return kept, used, over or rows < n_lim, rows


def expected_list(T, pairs, c, terrain, hits, n_lim, kmax, single=False):
    """the contact list of one env: terrain entries as given, then the self-collision entries of `hits` (pair indices, ascending)"""
    rad = T.rad32 if single else T.col_radius
    kept, count, over, rows = assemble(len(terrain), hits, n_lim, kmax)
    ids, bodies, pos, nrm, dep = [list(terrain[k]) for k in ("collision", "body", "position", "normal", "depth")]
    for h in kept:
        i, j = pairs[h]
        d = c[i] - c[j]
        dist = np.linalg.norm(d)
        n, depth = d / dist, rad[i] + rad[j] - dist
        x = c[i] - (rad[i] - 0.5 * depth) * n
        ids += [i | SELF_A, j | SELF_B]; bodies += [T.col_body[i], T.col_body[j]]
        pos += [x, x]; nrm += [n, -n]; dep += [depth, depth]
    return dict(ids=np.array(ids, np.int64), bodies=np.array(bodies, np.int64), pos=np.array(pos, np.float64).reshape(-1, 3),
                nrm=np.array(nrm, np.float64).reshape(-1, 3), dep=np.array(dep, np.float64), count=count, flag=int(over), rows=rows,
                nself=len(kept), n0=len(terrain), rows_wanted=n_lim, d_hit=[float(np.linalg.norm(c[pairs[h, 0]] - c[pairs[h, 1]])) for h in kept])


WORST_KEYS = ("position", "depth", "normal", "unit")


def compare(T, pairs, q, cnt, con, flag, kmax, n_lim, tie, bar, unit, d_min, single=False, perturb=None):
    """One env's reported list (cnt, con: structured array with position / normal / depth / body / collision; flag: rsb_get_flags' word) against the
    reference at state q.  A pair with | dist - (r_i + r_j) | < tie may be reported or not.  -> (failure or None, worst errors, pairs in the tie band,
    the expected list that matched - the first one tried if none did)
    perturb(expected) edits the expected list first: the sensitivity checks."""
    c = centres(T, q, single)
    dist, rs = pair_distances(T, pairs, c, single)
    live = dist * dist >= COINCIDENT2
    tied = np.nonzero(live & (np.abs(dist - rs) < tie))[0]
    sure = [int(h) for h in np.nonzero(live & (dist < rs) & (np.abs(dist - rs) >= tie))[0]]
    assert len(tied) <= 3
    con = con[:cnt]
    n0 = 0
    while n0 < cnt and con["collision"][n0] < SELF_A:
        n0 += 1
    terrain = con[:n0]
    first = first_ex = None
    for mask in range(1 << len(tied)):
        hits = sorted(sure + [int(t) for k, t in enumerate(tied) if mask >> k & 1])
        ex = expected_list(T, pairs, c, terrain, hits, n_lim, kmax, single)
        if perturb is not None:
            perturb(ex)
        why, worst = _compare_lists(ex, cnt, con, flag, bar, unit, d_min)
        if why is None:
            return None, worst, len(tied), ex
        first, first_ex = first or why, first_ex or ex
    return first, dict.fromkeys(WORST_KEYS, 0.0), len(tied), first_ex


def _compare_lists(ex, cnt, con, flag, bar, unit, d_min):
    worst = dict.fromkeys(WORST_KEYS, 0.0)
    if cnt != ex["count"]:
        return f"count {cnt}, expected {ex['count']}", worst
    if (flag & 1) != ex["flag"]:
        return f"overflow bit {flag & 1}, expected {ex['flag']}", worst
    if not np.array_equal(con["collision"], ex["ids"]):
        return f"ids {[hex(i) for i in con['collision']]}, expected {[hex(i) for i in ex['ids']]}", worst
    if not np.array_equal(con["body"], ex["bodies"]):
        return f"bodies {con['body']}, expected {ex['bodies']}", worst
    s = slice(ex["n0"], cnt)
    if cnt > ex["n0"]:
        worst["position"] = float(np.abs(con["position"][s] - ex["pos"][s]).max())
        worst["depth"] = float(np.abs(con["depth"][s] - ex["dep"][s]).max())
        worst["normal"] = float(np.abs(con["normal"][s] - ex["nrm"][s]).max())
        worst["unit"] = float(np.abs(np.linalg.norm(con["normal"][s].astype(np.float64), axis=1) - 1.0).max())
        if min(ex["d_hit"]) < d_min:
            return f"a designed hit's centres are {min(ex['d_hit']):.3g} apart, below d_min", worst
        nbar = 2.0 * bar / d_min
        for key, lim in (("position", bar), ("depth", bar), ("normal", nbar), ("unit", unit)):
            if not worst[key] <= lim:
                return f"{key} off by {worst[key]:.3g} (bar {lim:.3g})", worst
    return None, worst


# ---- the sensitivity checks' perturbations of the expected list ---------------------------------------------------------------------------------
def swap_two_hits(ex):
    a = ex["n0"]
    if ex["nself"] >= 2:
        for k in ("ids", "bodies", "pos", "nrm", "dep"):
            ex[k][[a, a + 1, a + 2, a + 3]] = ex[k][[a + 2, a + 3, a, a + 1]]


def flip_a_normal(ex):
    if ex["nself"]:
        ex["nrm"][ex["n0"]] *= -1.0


def point_on_the_surface_of_i():
    def f(ex):
        for k in range(ex["nself"]):      # c_i - r_i n instead of the middle of the overlap
            a = ex["n0"] + 2 * k
            ex["pos"][a] = ex["pos"][a + 1] = ex["pos"][a] - 0.5 * ex["dep"][a] * ex["nrm"][a]
    return f


def odd_slot_withheld(kmax):
    def f(ex):      # as if a limit row could not take the slot that is left when the self-collisions have taken theirs two by two
        if (kmax - ex["n0"]) % 2 == 1:
            ex["rows"] = min(ex["rows_wanted"], kmax - ex["count"] - 1)
            ex["flag"] = int(ex["flag"] or ex["rows"] < ex["rows_wanted"])
    return f


def drop_the_last_pair(last_pair):
    def f(ex):
        if ex["nself"] and (ex["ids"][-2] & 0xffff, ex["ids"][-1] & 0xffff) == tuple(last_pair):
            for k in ("ids", "bodies", "pos", "nrm", "dep"):
                ex[k] = ex[k][:-2]
            ex["count"] -= 2; ex["nself"] -= 1; ex["d_hit"] = ex["d_hit"][:-1] or [1.0]
    return f


# ---- designed models ------------------------------------------------------------------------------------------------------------------------------
def _xyz(v):
    return " ".join(repr(float(x)) for x in v)      # repr() round-trips the doubles


def _link(name, mass, spheres, extra=""):
    i = 0.4 * mass * 0.05 * 0.05
    cols = "".join(f'    <collision><origin xyz="{_xyz(p)}"/><geometry><sphere radius="{float(r)!r}"/></geometry></collision>\n' for p, r in spheres)
    return (f'  <link name="{name}">\n    <inertial><origin xyz="0 0 0"/><mass value="{mass}"/><inertia ixx="{i}" ixy="0" ixz="0" iyy="{i}" iyz="0" izz="{i}"/></inertial>\n'
            f'{cols}{extra}  </link>\n')


def _joint(name, kind, parent, child, origin, axis, lower, upper):
    return (f'  <joint name="{name}" type="{kind}"><origin xyz="{_xyz(origin)}"/><parent link="{parent}"/><child link="{child}"/>'
            f'<axis xyz="{_xyz(axis)}"/><limit effort="0" velocity="100" lower="{lower}" upper="{upper}"/></joint>\n')


HINGE, RHO, GAP = -0.1, 0.09, 0.14      # hinge's place on its limb's line, first elbow sphere's radius arm, spacing of a limb's spheres
LOCAL_MAX = 0.72                       # every centre of a placement stays this close to the base origin (base translations <= 0.25: coordinates within 1 m)
ELBOW_LIMIT = 3.3                        # rad; an elbow at 3.35 is the same pose as at 3.35 - 2 pi, and a joint past its limit


class Comb:
    """base (spheres `n_base`) + limbs: limb k has limb_counts[k] spheres on its slide line and an elbow with elbow_counts[k] spheres.  shapes (model C): limb 0 also carries a
    capsule and a cylinder laid along its line behind its spheres, limbs 1 and 2 a 4 cm box each (eight zero-radius corner points).  Radii 0.027 .. 0.032 m, all different (so a ground plane can single out the n largest)."""

    def __init__(self, n_base, limb_counts, elbow_counts, seed, shapes=False):
        rng = np.random.default_rng(seed)
        L = len(limb_counts)
        self.L, self.rng = L, rng
        n_sph = n_base + sum(limb_counts) + sum(elbow_counts)
        radii = list(np.round(0.027 + 0.005 * rng.permutation(n_sph) / max(n_sph - 1, 1), 5))
        while True:      # L lines in the plane, their crossings within 0.35 m of the centre and >= 0.1 m from each other
            ang = (np.arange(L) * np.pi / L + rng.uniform(-0.12, 0.12, L)) + rng.uniform(0, np.pi)
            self.a = np.round(np.c_[np.cos(ang), np.sin(ang)], 6)
            self.a /= np.linalg.norm(self.a, axis=1, keepdims=True)
            self.o = np.round(rng.uniform(-0.12, 0.12, (L, 2)), 4)
            self.X = {(k, m): self._cross(self.o[k], self.a[k], self.o[m], self.a[m]) for k in range(L) for m in range(k + 1, L)}
            pts = np.array(list(self.X.values()))
            dd = np.linalg.norm(pts[:, None] - pts[None], axis=2) + 10.0 * np.eye(len(pts))
            if np.abs(pts).max() < 0.35 and dd.min() > 0.1:
                break
        self.n = np.c_[-self.a[:, 1], self.a[:, 0]]
        # the base's spheres: beside a crossing, 0.05 m along the bisector - inside the bands of both lines; sphere b at crossing (2b, 2b + 1) mod L
        self.base_at = [((2 * b) % L, (2 * b + 1) % L) for b in range(n_base)]
        parts = ['<?xml version="1.0"?>\n<robot name="comb">\n']
        base = []
        for b, (k, m) in enumerate(self.base_at):
            bis = self.a[k] + self.a[m] * (1 if b % 2 == 0 else -1)
            base.append((np.round(np.r_[self._x(k, m) + 0.05 * bis / np.linalg.norm(bis), 0.0], 4), radii.pop()))
        parts.append(_link("base", 8.0, base))
        self.limits = {}
        for k in range(L):
            limb = [(np.r_[i * GAP * self.a[k], 0.0], radii.pop()) for i in range(limb_counts[k])]
            extra = ""
            if shapes and k == 0:      # axes along the line: rpy = (0, pi / 2, yaw of a_k) turns the shape's z axis into (a_k, 0)
                yaw, at = np.arctan2(self.a[k][1], self.a[k][0]), len(limb) * GAP
                self.capsule_at, self.cylinder_at = at + 0.5 * GAP, at + 2.0 * GAP
                extra = (f'    <collision><origin xyz="{_xyz(np.r_[self.capsule_at * self.a[k], 0.0])}" rpy="0 {np.pi / 2!r} {float(yaw)!r}"/><geometry><capsule radius="0.0285" length="{GAP}"/></geometry></collision>\n'
                         f'    <collision><origin xyz="{_xyz(np.r_[self.cylinder_at * self.a[k], 0.0])}" rpy="0 {np.pi / 2!r} {float(yaw)!r}"/><geometry><cylinder radius="0.03" length="0.08"/></geometry></collision>\n')
            elif shapes and k in (1, 2):
                extra = f'    <collision><origin xyz="{_xyz(np.r_[(len(limb) * GAP + 0.03) * self.a[k], 0.0])}"/><geometry><box size="0.04 0.04 0.04"/></geometry></collision>\n'
            parts.append(_link(f"limb{k}", 1.0, limb, extra))
            elbow = [(np.r_[(RHO + 0.07 * i) * self.a[k], 0.0], radii.pop()) for i in range(elbow_counts[k])]
            parts.append(_link(f"elbow{k}", 0.3, elbow))
            parts.append(_joint(f"slide{k}", "prismatic", "base", f"limb{k}", np.r_[self.o[k], 0.0], np.r_[self.a[k], 0.0], -3.0, 3.0))
            parts.append(_joint(f"hinge{k}", "revolute", f"limb{k}", f"elbow{k}", np.r_[HINGE * self.a[k], 0.0], (0.0, 0.0, 1.0), -ELBOW_LIMIT, ELBOW_LIMIT))
        parts.append("</robot>\n")
        self.urdf = "".join(parts)
        self.limb_body = [1 + 2 * k for k in range(L)]
        self.elbow_body = [2 + 2 * k for k in range(L)]
        for k in range(L):
            self.limits[self.limb_body[k]] = (-3.0, 3.0)
            self.limits[self.elbow_body[k]] = (-ELBOW_LIMIT, ELBOW_LIMIT)

    @staticmethod
    def _cross(o1, a1, o2, a2):
        t = np.linalg.solve(np.c_[a1, -a2], o2 - o1)
        return o1 + t[0] * a1

    def _x(self, k, m):
        return self.X[(min(k, m), max(k, m))]

    def bind(self, blob):
        """the loaded model's tables; checks that the loader numbered bodies as the design assumes (by the joint origins and types alone)"""
        T = Tables(blob)
        self.T = T
        assert T.nb == 1 + 2 * self.L
        for k in range(self.L):
            lb, eb = self.limb_body[k], self.elbow_body[k]
            assert T.parent[lb] == 0 and T.jtype[lb] == PRISMATIC and np.allclose(T.origin[lb][:2], self.o[k]) and np.allclose(T.axis[lb][:2], self.a[k])
            assert T.parent[eb] == lb and T.jtype[eb] == REVOLUTE
        self.pairs = candidate_pairs(T)
        self.nq = 7 + 2 * self.L
        self.home = self._find_home()
        return T

    # -- local (base-frame, identity pose) geometry ------------------------------------------------------------------------------------------------
    def local_q(self, joints):
        return np.r_[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, joints]

    def gaps(self, joints, pairs=None):
        pairs = self.pairs if pairs is None else pairs
        d, rs = pair_distances(self.T, pairs, centres(self.T, self.local_q(joints)))
        return d - rs

    def _find_home(self):
        """every limb parked where all candidate pairs are farthest apart: random search, elbows folded back along their lines"""
        best, best_gap = None, -1.0
        for _ in range(1500):
            j = np.zeros(2 * self.L)
            j[0::2] = self.rng.uniform(0.25, 0.5, self.L) * self.rng.choice([-1.0, 1.0], self.L) - GAP
            j[1::2] = (self.rng.choice([0.0, np.pi], self.L) + self.rng.uniform(-0.5, 0.5, self.L) + np.pi) % (2 * np.pi) - np.pi
            if np.abs(centres(self.T, self.local_q(j))).max() > LOCAL_MAX:
                continue
            g = self.gaps(j).min()
            if g > best_gap:
                best, best_gap = j, g
        assert best_gap > 0.03, best_gap
        return best

    def kind(self, prim):
        b = self.T.col_body[prim]
        return ("base", -1) if b == 0 else ("limb", (b - 1) // 2) if b % 2 == 1 else ("elbow", (b - 2) // 2)

    def _put_limb(self, j, k, prim, point):
        """slide limb k so that its sphere `prim` (on the line) is at the foot of `point` on the line"""
        j[2 * k] = (point - self.o[k]) @ self.a[k] - self.T.col_pos[prim][:2] @ self.a[k]

    def _put_elbow(self, j, k, prim, point, branch):
        """slide limb k and turn its elbow so that the elbow's sphere `prim` is at `point` (within its arm of line k); False if out of reach"""
        arm = self.T.col_pos[prim][:2] @ self.a[k]
        perp = (point - self.o[k]) @ self.n[k]
        if abs(perp) > 0.95 * arm:
            return False
        th = np.arcsin(perp / arm)
        th = np.pi - th if branch else th
        j[2 * k + 1] = (th + np.pi) % (2 * np.pi) - np.pi
        j[2 * k] = (point - self.o[k]) @ self.a[k] - arm * np.cos(th) - HINGE
        return True

    def _try_pair(self, j, p, d):
        """one random closed-form try at bringing pair p's centres d apart; edits joints j; False if this try is geometrically impossible"""
        rng = self.rng
        i, jj = self.pairs[p]
        (ki, li), (kj, lj) = self.kind(i), self.kind(jj)
        u = rng.normal(size=2); u /= np.linalg.norm(u)
        if ki == "base":      # base sphere x elbow
            assert kj == "elbow"
            return self._put_elbow(j, lj, jj, self.T.col_pos[i][:2] + d * u, rng.integers(2))
        if ki == "limb" and kj == "limb":
            X = self._x(li, lj)
            self._put_limb(j, lj, jj, X)
            self._put_limb(j, li, i, X + d * rng.choice([-1.0, 1.0]) * self.a[li])
            return True
        if {ki, kj} == {"limb", "elbow"}:
            (lk, lprim), (ek, eprim) = ((li, i), (lj, jj)) if ki == "limb" else ((lj, jj), (li, i))
            s = np.sqrt(max(1.0 - (self.a[lk] @ self.a[ek]) ** 2, 1e-9))
            P = self._x(lk, ek) + rng.choice([-1.0, 1.0]) * rng.uniform(0.045, 0.075) / s * self.a[lk]      # on line lk, 0.045 .. 0.075 from line ek
            self._put_limb(j, lk, lprim, P)
            return self._put_elbow(j, ek, eprim, P + d * u, rng.integers(2))
        assert ki == kj == "elbow"
        Pi = self._x(li, lj) + rng.uniform(-0.09, 0.09, 2)
        return self._put_elbow(j, li, i, Pi, rng.integers(2)) and self._put_elbow(j, lj, jj, Pi + d * u, rng.integers(2))

    def limbs_of(self, p):
        return {self.kind(s)[1] for s in self.pairs[p]} - {-1}

    def place(self, targets, clear=1e-3, tries=600, fixed=None):
        """joints at which the pairs of `targets` = {pair: overlap} have r_i + r_j - dist = overlap (> 0: a hit whose centres are >= 0.05 m apart; < 0: a miss
        by that gap; None: coincident centres) and every other pair is at least `clear` apart.  The targets' limbs must be disjoint.
        fixed: {joint index: value} of idle limbs, set before the check."""
        used = [self.limbs_of(p) for p in targets]
        assert sum(map(len, used)) == len(set().union(*used)), "targets share a limb"
        busy = set().union(*used)
        for t in range(tries):
            j = self.home.copy()
            for k in range(self.L):      # other choices for what the closed forms leave free: the elbows of the targets' limbs; later also where the idle limbs park
                if k in busy:
                    j[2 * k + 1] = self.rng.uniform(-np.pi, np.pi)
                elif t >= 20 and self.rng.random() < 0.5:
                    j[2 * k:2 * k + 2] = self.rng.uniform(0.25, 0.5) * self.rng.choice([-1.0, 1.0]) - GAP, self.rng.uniform(-np.pi, np.pi)
            for i, v in (fixed or {}).items():
                j[i] = v
            ok = True
            for p, ov in targets.items():
                ok = self._coincide(j, p) if ov is None else (self._try_pair(j, p, self.T.col_radius[self.pairs[p]].sum() - ov) and self._polish(j, p, self.T.col_radius[self.pairs[p]].sum() - ov))
                if not ok:
                    break
            if not ok:
                continue
            d, rs = pair_distances(self.T, self.pairs, centres(self.T, self.local_q(j)))
            rest = np.ones(len(d), bool)
            for p, ov in targets.items():
                rest[p] = False
                ok = ok and (d[p] < 1e-9 if ov is None else abs(rs[p] - d[p] - ov) < 1e-10 and (ov < 0 or d[p] >= 0.0505 or d[p] < 1e-6))
            if not ok or (d - rs)[rest].min() < clear or np.abs(centres(self.T, self.local_q(j))).max() > LOCAL_MAX:
                continue
            return j
        raise AssertionError(f"no placement for {targets}")

    def _coincide(self, j, p):
        i, jj = self.pairs[p]
        (ki, li), (kj, lj) = self.kind(i), self.kind(jj)
        if ki == "limb" and kj == "limb":
            X = self._x(li, lj)
            self._put_limb(j, li, i, X); self._put_limb(j, lj, jj, X)
            return True
        if ki == "base":
            return self._put_elbow(j, lj, jj, self.T.col_pos[i][:2], self.rng.integers(2))
        return False

    def _polish(self, j, p, d):
        """secant steps on the slide of one of the pair's limbs until the centre distance is d to 1e-12"""
        k = max(self.limbs_of(p))
        pr = self.pairs[p:p + 1]

        def f(x):
            jx = j.copy(); jx[2 * k] = x
            return pair_distances(self.T, pr, centres(self.T, self.local_q(jx)))[0][0] - d
        x0, x1 = j[2 * k], j[2 * k] + 1e-6
        f0, f1 = f(x0), f(x1)
        for _ in range(30):
            if abs(f1) < 1e-13 or f1 == f0:
                break
            x0, x1, f0 = x1, x1 - f1 * (x1 - x0) / (f1 - f0), f1
            f1 = f(x1)
        if abs(f1) > 1e-11 or abs(x1 - j[2 * k]) > 1e-2:
            return False
        j[2 * k] = x1
        return True


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def yaw_quat(angle):
    return np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])


# ---- closed forms of the material tests -------------------------------------------------------------------------------------------------------------
def head_on(m_a, m_b, v_a, v_b, e, thr):
    """two bodies on one line, A behind B (v_a > v_b: approaching): velocities after the impact.  Momentum is conserved; the relative speed v_a - v_b becomes
    -e times itself where the approach speed exceeds thr, 0 where it does not."""
    rel = v_a - v_b
    rel_after = -e * rel if rel > thr else 0.0
    vc = (m_a * v_a + m_b * v_b) / (m_a + m_b)
    return vc + m_b / (m_a + m_b) * rel_after, vc - m_a / (m_a + m_b) * rel_after


def tangential(m_a, v_a, m_b, v_t, mu, e, thr):
    """A (speed v_a along the line of centres) is stopped by B, which cannot move along that line: J_n = m_a v_a (1 + e) (e counts above thr only).  B slides
    along a tangent with v_t.  -> (v_a after, v_t after, regime): 'slip' m_b |v_t| > 2 mu J_n: v_t loses mu J_n / m_b; 'stick' m_b |v_t| < mu J_n / 2: v_t = 0;
    None in between (not asserted)."""
    ee = e if v_a > thr else 0.0
    jn = m_a * v_a * (1.0 + ee)
    if m_b * abs(v_t) > 2.0 * mu * jn:
        return -ee * v_a, v_t - np.sign(v_t) * mu * jn / m_b, "slip"
    if m_b * abs(v_t) < 0.5 * mu * jn:
        return -ee * v_a, 0.0, "stick"
    return -ee * v_a, None, None


def couples_urdf(K, masses_a, masses_b, tangent):
    """fixed base `world` + K couples of sliders, couple k at y = 0.3 k: A_k slides along x; B_k along x (head-on) or along y (tangent); one sphere r = 0.05 each.
    At q = 0, A_k is at x = 0 and B_k at x = 0.25: apart."""
    parts = ['<?xml version="1.0"?>\n<robot name="couples">\n', _link("world", 1.0, [])]
    for k in range(K):
        parts.append(_link(f"a{k}", masses_a[k], [((0.0, 0.0, 0.0), 0.05)]))
        parts.append(_link(f"b{k}", masses_b[k], [((0.0, 0.0, 0.0), 0.05)]))
        parts.append(_joint(f"ja{k}", "prismatic", "world", f"a{k}", (0.0, 0.3 * k - 0.75, 0.0), (1.0, 0.0, 0.0), -5.0, 5.0))
        parts.append(_joint(f"jb{k}", "prismatic", "world", f"b{k}", (0.25, 0.3 * k - 0.75, 0.0), (0.0, 1.0, 0.0) if tangent else (1.0, 0.0, 0.0), -5.0, 5.0))
    parts.append("</robot>\n")
    return "".join(parts)


# ---- designed worlds: N = 64 states of one comb, one family of placements per group of envs ---------------------------------------------------------------
N_ENVS, LANES = 64, (16, 32, 64)
MODEL_A = dict(n_base=2, limb_counts=[3] * 5, elbow_counts=[1] * 5, seed=1)            # 170 candidate pairs
MODEL_B = dict(n_base=2, limb_counts=[2, 2, 2, 1], elbow_counts=[1, 1, 1, 2], seed=2)  # exactly 64
MODEL_C = dict(n_base=1, limb_counts=[2, 2, 2], elbow_counts=[1, 1, 1], seed=3, shapes=True)
OVERLAP = 1e-3


class Scene:
    """q [N, nq] (already float32-rounded), per env: label, the joints past their limit; kmax; ground height or None; ignored body pairs"""

    def __init__(self, comb, kmax=16, ground=None, ignore=(), erp=0.0):
        self.comb, self.kmax, self.ground, self.ignore, self.erp = comb, kmax, ground, list(ignore), erp
        self.q = np.zeros((N_ENVS, comb.nq))
        self.label = [None] * N_ENVS
        self.targets = [None] * N_ENVS
        self.n_lim = np.zeros(N_ENVS, int)
        self.lim_joint = [None] * N_ENVS      # (body, sign of the limit row) of the joint past its limit
        self.free = list(range(0, N_ENVS, 2))      # even envs carry the designed hits, every odd env hits nothing: mixed lanes in every wave

    def put(self, e, label, joints, p, quat, targets=None, lim=None):
        self.q[e] = np.r_[p, quat, joints]
        self.label[e], self.targets[e] = label, dict(targets or {})
        if lim is not None:
            self.n_lim[e], self.lim_joint[e] = 1, lim

    def add(self, label, joints, p, quat, targets=None, lim=None):
        e = self.free.pop(0)
        self.put(e, label, joints, p, quat, targets, lim)
        return e

    def finish(self):
        assert all(l is not None for l in self.label)
        self.q = f32(self.q)
        assert all(self.n_lim[e] == limit_rows(self.q[e], self.comb.limits) for e in range(N_ENVS))      # exactly the designed joints are past their limits
        return self


def _pose(rng):
    return rng.uniform(-0.25, 0.25, 3), random_quat(rng)


def _fill_misses(sc, rng, pairs_for_near, flat=False):
    """every env still without a state hits nothing: parked, or with one pair a designed gap (1e-4 .. 1e-3 m) short of touching"""
    comb = sc.comb
    gaps = (1e-4, 3e-4, 1e-3)
    for n, e in enumerate([e for e in range(N_ENVS) if sc.label[e] is None]):
        p, quat = _pose(rng)
        if flat:
            p, quat = np.r_[p[:2], 0.1], yaw_quat(rng.uniform(-np.pi, np.pi))      # (0.1 m above the ground: no terrain contact either)
        if n % 3 == 2:
            j = comb.home.copy()
            j[1::2] = (j[1::2] + rng.uniform(-0.2, 0.2, comb.L) + np.pi) % (2 * np.pi) - np.pi
            assert comb.gaps(j).min() >= 1e-3
            sc.put(e, "miss: parked", j, p, quat)
        else:
            pr = int(pairs_for_near[n % len(pairs_for_near)])
            g = gaps[n % 3]
            sc.put(e, f"miss: pair {pr} short by {g:g}", comb.place({pr: -g}), p, quat, {pr: -g})


def disjoint_sets(comb, rng, size, ok, tries=20000):
    """`size` pairs on pairwise different limbs for which ok(tuple of pairs) holds, and their placement"""
    n = len(comb.pairs)
    placeable = [p for p in range(n) if comb.kind(comb.pairs[p][0])[0] != "base" or _in_band(comb, p)]
    for _ in range(tries):
        ps = tuple(sorted(int(x) for x in rng.choice(placeable, size, replace=False)))
        limbs = [comb.limbs_of(p) for p in ps]
        if sum(map(len, limbs)) != len(set().union(*limbs)) or not ok(ps):
            continue
        try:
            return ps, comb.place({p: OVERLAP for p in ps}, tries=60)
        except AssertionError:
            continue
    raise AssertionError("no such set of pairs")


def _in_band(comb, p):
    i, j = comb.pairs[p]
    return comb.kind(j)[1] in comb.base_at[i]


def scene_main(comb, seed, with_families=True):
    """families 1 (single hits at the ends of the list and on both sides of every pass boundary), 2 (several passes, two in one pass), 3 (misses),
    4 (coincident centres) and the grazing family"""
    rng = np.random.default_rng(seed)
    sc = Scene(comb)
    n = len(comb.pairs)
    singles = sorted({0, n - 1} | {b for l in LANES for b in (l - 1, l) if b < n})
    for pr in singles:
        sc.add(f"single: pair {pr}", comb.place({pr: OVERLAP}), *_pose(rng), {pr: OVERLAP})
    if with_families:
        three, j3 = disjoint_sets(comb, rng, 3, lambda ps: len({p // 64 for p in ps}) == 3)
        sc.add(f"three passes: pairs {three}", j3, *_pose(rng), {p: OVERLAP for p in three})
        for _ in range(2):
            two, j2 = disjoint_sets(comb, rng, 2, lambda ps: ps[0] // 64 != ps[1] // 64)
            sc.add(f"two passes: pairs {two}", j2, *_pose(rng), {p: OVERLAP for p in two})
        for _ in range(2):
            one, j1 = disjoint_sets(comb, rng, 2, lambda ps: ps[0] // 16 == ps[1] // 16)
            sc.add(f"one pass: pairs {one}", j1, *_pose(rng), {p: OVERLAP for p in one})
        # coincident centres: limb sphere on limb sphere where their lines cross.  The pose is exact in float32 (no rotation, no translation), so the centre
        # distance the device computes stays below the 1e-6 guard: <= 4 roundings of 3e-8 (half an ulp below 0.5 m) per centre
        limb_pairs = [p for p in range(n) if comb.kind(comb.pairs[p][0])[0] == "limb" and comb.kind(comb.pairs[p][1])[0] == "limb"]
        ident = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))
        for near, with_hit in ((None, False), (5e-7, False), (None, True), (5e-7, True)):
            while True:
                pc = int(rng.choice(limb_pairs))
                tg = {pc: None if near is None else float(comb.T.col_radius[comb.pairs[pc]].sum() - near)}
                if with_hit:
                    other = [p for p in limb_pairs if not comb.limbs_of(p) & comb.limbs_of(pc)]
                    tg[int(rng.choice(other))] = OVERLAP
                try:
                    j = comb.place(tg, tries=100)
                    break
                except AssertionError:
                    continue
            sc.add(f"coincident: pair {pc} at {near or 0:g}" + (" beside a hit" if with_hit else ""), j, *ident, tg)
        for k, ov in enumerate(np.geomspace(1e-7, 1e-5, 8)):      # grazing: the only family allowed to use the tie-band exclusion
            pr = int(rng.integers(n))
            while comb.kind(comb.pairs[pr][0])[0] == "base" and not _in_band(comb, pr):
                pr = int(rng.integers(n))
            sc.add(f"grazing: pair {pr} by {ov:.1e}", comb.place({pr: float(ov)}), *_pose(rng), {pr: float(ov)})
    _fill_misses(sc, rng, rng.permutation([p for p in range(n) if comb.kind(comb.pairs[p][0])[0] != "base" or _in_band(comb, p)]))
    return sc.finish()


OVERFLOW_CASES = {      # kmax: (terrain contacts n0, hits, what happens to the last hit)
    8: ((2, 3, "fits exactly"), (3, 3, "misses by one slot"), (2, 4, "misses by two slots"), (3, 2, "fits, one odd slot left")),
    5: ((1, 2, "fits exactly"), (2, 2, "misses by one slot"), (1, 3, "misses by two slots"), (0, 2, "fits, one odd slot left")),
    16: ((10, 3, "fits exactly"), (11, 3, "misses by one slot"), (10, 4, "misses by two slots"), (11, 2, "fits, one odd slot left")),
}
PAST_LIMIT = 0.05      # rad beyond the elbow's range


def scene_overflow(comb, kmax, seed):
    """family 5: on a ground plane at z = 0 with the comb's plane level at height z, the n0 largest spheres (r > z) touch the ground and come first; then
    hits on different limbs; each case once with an idle limb's elbow PAST_LIMIT beyond its range and once without"""
    rng = np.random.default_rng(seed)
    sc = Scene(comb, kmax=kmax, ground=0.0, erp=0.2)
    n = len(comb.pairs)
    r_sorted = np.sort(comb.T.rad32)[::-1]
    assert (np.diff(r_sorted) < -2e-4).all()
    one_limb = [p for p in range(n) if comb.kind(comb.pairs[p][0])[0] == "base" and _in_band(comb, p)]      # base x elbow: four hits fit on four limbs
    used = {}      # envs of one wave (four consecutive envs at 16 lanes) must differ in which pairs hit
    for lim in (False, True):
        for n0, h, what in OVERFLOW_CASES[kmax]:
            z = 0.5 * (r_sorted[n0 - 1] + r_sorted[n0]) if n0 else r_sorted[0] + 1.2e-4
            while True:
                ps = tuple(sorted(int(x) for x in rng.choice(one_limb, h, replace=False)))
                limbs = set().union(*[comb.limbs_of(p) for p in ps])
                if len(limbs) != h or ps in used.get(sc.free[0] // 4, ()):
                    continue
                idle = [k for k in range(comb.L) if k not in limbs]
                sgn = float(rng.choice([-1.0, 1.0]))
                fixed = {2 * idle[0] + 1: sgn * (ELBOW_LIMIT + PAST_LIMIT)} if lim else {}
                try:
                    j = comb.place({p: OVERLAP for p in ps}, tries=60, fixed=fixed)
                    break
                except AssertionError:
                    continue
            used.setdefault(sc.free[0] // 4, []).append(ps)
            sc.add(f"overflow kmax {kmax}: {n0} on the ground, {h} hits, the last {what}" + (", a joint past its limit" if lim else ""),
                   j, np.r_[rng.uniform(-0.25, 0.25, 2), z], yaw_quat(rng.uniform(-np.pi, np.pi)), {p: OVERLAP for p in ps},
                   (comb.elbow_body[idle[0]], -sgn) if lim else None)
    _fill_misses(sc, rng, rng.permutation(one_limb), flat=True)
    return sc.finish()


def scene_ignore(comb, seed):
    """family 6: two hits per env on different limbs; the test ignores the body pair of one of them (sc.ignore)"""
    rng = np.random.default_rng(seed)
    n = len(comb.pairs)
    limb_pairs = [p for p in range(n) if comb.kind(comb.pairs[p][0])[0] == "limb" and comb.kind(comb.pairs[p][1])[0] == "limb"]
    p_ign = int(rng.choice(limb_pairs))
    sc = Scene(comb, ignore=[tuple(int(comb.T.col_body[s]) for s in comb.pairs[p_ign])])
    same_bodies = [p for p in limb_pairs if {int(comb.T.col_body[s]) for s in comb.pairs[p]} == set(sc.ignore[0])]
    others = [p for p in range(n) if not comb.limbs_of(p) & comb.limbs_of(p_ign) and (comb.kind(comb.pairs[p][0])[0] != "base" or _in_band(comb, p))]
    for k in range(8):
        while True:
            tg = {int(rng.choice(same_bodies)): OVERLAP, int(rng.choice(others)): OVERLAP}
            try:
                j = comb.place(tg, tries=60)
                break
            except AssertionError:
                continue
        sc.add(f"ignore: pairs {sorted(tg)}, the first on the ignored bodies", j, *_pose(rng), tg)
    _fill_misses(sc, rng, rng.permutation(others))
    return sc.finish()


class Tally:
    """worst value per quantity over every env checked, and how many (env, pair) placements sat in the tie band"""

    def __init__(self):
        self.worst = dict.fromkeys(WORST_KEYS, 0.0)
        self.placements = self.tied = self.envs = self.hits = 0
        self.failures = []

    def lines(self):
        w = self.worst
        return [f"{self.envs} envs, {self.placements} (env, pair) placements, {self.hits} self-collisions, {self.tied} in the tie band: position {w['position']:.2e} m, "
                f"depth {w['depth']:.2e} m, normal {w['normal']:.2e}, | |n| - 1 | {w['unit']:.2e}"]


def check_scene(sc, T, pairs, cnt, con, flags, u, tie, bar, unit, single, tally, perturb=None, dt=0.0025, name=""):
    """every env of a scene against the reference; the envs with a joint past its limit also by what the limit row does: with erp > 0 a row that got a
    slot leaves its joint moving back at erp * violation / dt (4 rad/s here), a row without one leaves it where the self-collisions' recoil puts it (far below
    1 rad/s).  -> the expected lists, env by env"""
    out = []
    for e in range(N_ENVS):
        why, worst, n_tie, ex = compare(T, pairs, sc.q[e], int(cnt[e]), con[e], int(flags[e]), sc.kmax, int(sc.n_lim[e]), tie, bar, unit, 0.05, single, perturb)
        out.append(ex)
        tally.envs += 1; tally.placements += len(pairs); tally.tied += n_tie; tally.hits += ex["nself"]
        if why is not None:
            tally.failures.append(f"{name} env {e} ({sc.label[e]}): {why}")
            continue
        for k in WORST_KEYS:
            tally.worst[k] = max(tally.worst[k], worst[k])
        if sc.lim_joint[e] is not None and u is not None and sc.erp > 0:
            body, sgn = sc.lim_joint[e]
            v, full = sgn * float(u[e][5 + body]), sc.erp * PAST_LIMIT / dt
            if ex["rows"] and not v > 0.5 * full or not ex["rows"] and not abs(v) < 0.25 * full:
                tally.failures.append(f"{name} env {e} ({sc.label[e]}): limit row {'present' if ex['rows'] else 'absent'} but its joint moves back at {v:.3g} rad/s (a row gives {full:g})")
    return out


def scene_shapes(comb, seed):
    """model C: single hits on each of the capsule's two end spheres (two pairs per end); a sphere centred on either rim primitive of the cylinder reports
    nothing; the boxes' corner points are there for the candidate rule (point x point is no pair, point x sphere is one) and stay clear of everything"""
    rng = np.random.default_rng(seed)
    sc = Scene(comb)
    T, pairs = comb.T, comb.pairs
    caps = [s for s in range(T.ncol) if T.col_body[s] == comb.limb_body[0] and T.col_rim[s] == 0 and abs(abs(T.col_pos[s][:2] @ comb.a[0] - comb.capsule_at) - 0.5 * GAP) < 1e-9]
    rims = [s for s in range(T.ncol) if T.col_rim[s] > 0]
    assert len(caps) == 2 and len(rims) == 2 and (T.col_radius[caps] == 0.0285).all()
    sc.caps, sc.rims = caps, rims
    spheres = T.col_radius > 0
    for end in caps:
        for p in [p for p in range(len(pairs)) if end in pairs[p] and spheres[pairs[p]].all() and comb.kind(pairs[p][0])[0] == comb.kind(pairs[p][1])[0] == "limb"][:2]:
            sc.add(f"capsule end {end}: pair {p}", comb.place({p: OVERLAP}), *_pose(rng), {p: OVERLAP})
    for p in (0, len(pairs) - 1):
        sc.add(f"single: pair {p}", comb.place({p: OVERLAP}), *_pose(rng), {p: OVERLAP})
    for rim in rims:      # limb 1's first sphere on the rim primitive, where lines 0 and 1 cross
        first = int(np.nonzero(T.col_body == comb.limb_body[1])[0][0])
        for _ in range(200):
            j = comb.home.copy()
            j[3], j[1] = rng.uniform(-np.pi, np.pi, 2)
            comb._put_limb(j, 0, rim, comb._x(0, 1)); comb._put_limb(j, 1, first, comb._x(0, 1))
            c = centres(T, comb.local_q(j))
            if np.linalg.norm(c[rim] - c[first]) < 1e-9 and comb.gaps(j).min() >= 1e-3 and np.abs(c).max() <= LOCAL_MAX:
                break
        else:
            raise AssertionError("no placement on the rim primitive")
        sc.add(f"rim: sphere {first} centred on rim primitive {rim}", j, *_pose(rng))
    _fill_misses(sc, rng, [p for p in range(len(pairs)) if spheres[pairs[p]].all() and (comb.kind(pairs[p][0])[0] != "base" or _in_band(comb, p))])
    return sc.finish()


# ---- per-pair materials: K couples of sliders on a fixed base, each with its own (mu, restitution, threshold) ----------------------------------------
K_COUPLES = 6
MU = 0.15 * 1.3 ** np.array([0, 3, 1, 5, 2, 4])            # every couple's value differs from every other couple's by >= 30 % ...
REST = 0.9 / 1.3 ** np.array([2, 0, 5, 3, 1, 4])           # ... and the three orders differ, so no column can stand in for another
THR = 0.05 * 1.3 ** np.array([4, 1, 3, 0, 5, 2])           # m/s
MASS_A = np.array([1.0, 1.5, 2.0, 1.25, 0.8, 1.75])
MASS_B = np.array([2.0, 1.0, 1.2, 2.5, 1.6, 0.9])
FAST, SLOW = 1.15, 0.87      # approach speed / threshold: above its own threshold but below the next larger one (x 1.3), below its own but above the next smaller


class Couples:
    """states and closed-form expectations of the head-on (tangent = False) or friction (tangent = True) case.  Env e activates the couples in the bits of
    mask[e] (63 different non-empty subsets and one empty); couple k of env e approaches on the fast side of its threshold if (e + k) is even."""

    def __init__(self, tangent, blob):
        self.tangent = tangent
        T = Tables(blob)
        self.T = T
        self.body_a, self.body_b = [1 + 2 * k for k in range(K_COUPLES)], [2 + 2 * k for k in range(K_COUPLES)]
        for k in range(K_COUPLES):
            assert T.parent[self.body_a[k]] == 0 and T.parent[self.body_b[k]] == 0 and T.col_body[2 * k] == self.body_a[k] and T.col_body[2 * k + 1] == self.body_b[k]
        own = {frozenset((self.body_a[k], self.body_b[k])) for k in range(K_COUPLES)}
        self.ignore = [(a, b) for a in range(1, T.nb) for b in range(a + 1, T.nb) if frozenset((a, b)) not in own]
        self.pairs = candidate_pairs(T, self.ignore)
        assert np.array_equal(self.pairs, [(2 * k, 2 * k + 1) for k in range(K_COUPLES)])
        self.mask = np.array([(e * 37 + 11) % 63 + 1 for e in range(N_ENVS)])
        self.mask[63] = 0
        assert len(set(self.mask)) == N_ENVS
        self.active = np.array([[bool(m >> k & 1) for k in range(K_COUPLES)] for m in self.mask])
        self.fast = np.array([[(e + k) % 2 == 0 for k in range(K_COUPLES)] for e in range(N_ENVS)])
        self.slip = np.array([[(e // 2 + k) % 2 == 0 for k in range(K_COUPLES)] for e in range(N_ENVS)])
        for k in range(K_COUPLES):
            assert (self.active[:, k] & self.fast[:, k]).any() and (self.active[:, k] & ~self.fast[:, k]).any()
            if tangent:
                assert all((self.active[:, k] & (self.fast[:, k] == f) & (self.slip[:, k] == s)).any() for f in (0, 1) for s in (0, 1))

    def state(self, mu, rest, thr):
        """(q, u) and the expected u after one step under the materials given per couple"""
        q = np.zeros((N_ENVS, 7 + 2 * K_COUPLES)); q[:, 3] = 1.0
        u = np.zeros((N_ENVS, 6 + 2 * K_COUPLES))
        for e in range(N_ENVS):
            for k in range(K_COUPLES):
                if not self.active[e, k]:
                    continue
                q[e, 6 + self.body_a[k]] = 0.25 - (0.1 - OVERLAP)
                app = THR[k] * (FAST if self.fast[e, k] else SLOW)      # designed against the couple's OWN threshold, whatever materials the run uses
                if self.tangent:
                    jn = MASS_A[k] * app * (1.0 + (REST[k] if self.fast[e, k] else 0.0))
                    vt = (3.0 if self.slip[e, k] else 0.25) * MU[k] * jn / MASS_B[k] * (1.0 if (e + k) % 4 < 2 else -1.0)
                    u[e, 5 + self.body_a[k]], u[e, 5 + self.body_b[k]] = app, vt
                else:
                    u[e, 5 + self.body_a[k]], u[e, 5 + self.body_b[k]] = 0.7 * app, -0.3 * app
        q, u = f32(q), f32(u)
        want = u.copy()
        asserted = np.zeros((N_ENVS, K_COUPLES), bool)
        for e in range(N_ENVS):
            for k in range(K_COUPLES):
                if not self.active[e, k]:
                    continue
                ia, ib = 5 + self.body_a[k], 5 + self.body_b[k]
                if self.tangent:
                    va, vt, regime = tangential(MASS_A[k], u[e, ia], MASS_B[k], u[e, ib], mu[k], rest[k], thr[k])
                    want[e, ia] = va
                    want[e, ib] = u[e, ib] if vt is None else vt
                    asserted[e, k] = vt is not None
                else:
                    want[e, ia], want[e, ib] = head_on(MASS_A[k], MASS_B[k], u[e, ia], u[e, ib], rest[k], thr[k])
                    asserted[e, k] = True
        return q, u, want, asserted

    def errors(self, u1, want, asserted):
        """worst | u - closed form | over the asserted couples: (A's velocity, B's velocity, the sliders of inactive couples, which should stay at rest)"""
        ea = eb = ei = 0.0
        for e in range(N_ENVS):
            for k in range(K_COUPLES):
                ia, ib = 5 + self.body_a[k], 5 + self.body_b[k]
                if self.active[e, k]:
                    ea = max(ea, abs(u1[e, ia] - want[e, ia]))
                    if asserted[e, k]:
                        eb = max(eb, abs(u1[e, ib] - want[e, ib]))
                else:
                    ei = max(ei, abs(u1[e, ia]), abs(u1[e, ib]))
        return float(ea), float(eb), float(ei)

    def bars(self, u, want, solver_threshold=1e-5, reg=2e-4):
        """the closed forms' floor, derived: the solver stops at `solver_threshold`, and the Delassus block of a self-collision on a fixed base carries the compliance
        reg * trace / 3 on its diagonal (ORC_SELF_REG = kSelfReg = 1e-4, once for the self-collision and once for the fixed base), so a row with diagonal g
        delivers its impulse short by the fraction reg * trace / (3 g).  Head-on: trace = g_n = 1 / m_a + 1 / m_b.  Friction: trace = 1 / m_a + 1 / m_b, g_n = 1 / m_a,
        g_t = 1 / m_b.  -> (bar on A's velocity, bar on B's): threshold + the largest shortfall over the active couples"""
        ba = bb = 0.0
        for e in range(N_ENVS):
            for k in range(K_COUPLES):
                if not self.active[e, k]:
                    continue
                ia, ib = 5 + self.body_a[k], 5 + self.body_b[k]
                if self.tangent:
                    tr = 1.0 / MASS_A[k] + 1.0 / MASS_B[k]
                    ba = max(ba, reg * tr * MASS_A[k] / 3.0 * abs(want[e, ia] - u[e, ia]))
                    bb = max(bb, reg * tr * max(MASS_A[k], MASS_B[k]) / 3.0 * max(abs(want[e, ib] - u[e, ib]), abs(u[e, ib]) if want[e, ib] == 0.0 else 0.0))
                else:
                    ba, bb = max(ba, reg / 3.0 * abs(want[e, ia] - u[e, ia])), max(bb, reg / 3.0 * abs(want[e, ib] - u[e, ib]))
        return solver_threshold + ba, solver_threshold + bb


# ---- what the designed worlds reach, by the reference alone ------------------------------------------------------------------------------------------------
_CACHE = {}


def designed(name):
    """the designed models and scenes, built once per process: name -> (Comb, URDF-loaded Model, {scene name: Scene})"""
    if name not in _CACHE:
        from raisimlib_amd import Model
        comb = Comb(**{"A": MODEL_A, "B": MODEL_B, "C": MODEL_C}[name])
        model = Model(urdf_string=comb.urdf)
        comb.bind(model.blob)
        if name == "A":
            scenes = {"main": scene_main(comb, 10), "ignore": scene_ignore(comb, 30)}
            scenes.update({f"overflow {k}": scene_overflow(comb, k, 20 + k) for k in (8, 5, 16)})
        else:
            scenes = {"main": scene_main(comb, 11, with_families=False)} if name == "B" else {"shapes": scene_shapes(comb, 40)}
        _CACHE[name] = (comb, model, scenes)
    return _CACHE[name]


def scene_facts(sc, tie):
    """per env, from the reference alone (float32 primitive tables, as the device holds them): the sure hits, the pairs in the tie band, coincident pairs,
    the nearest gap of an env without hits, the terrain contacts the ground rule gives (c_z - r < ground), and what the assembly does with all that"""
    T = sc.comb.T
    pairs = candidate_pairs(T, sc.ignore)
    out = []
    for e in range(N_ENVS):
        c = centres(T, sc.q[e], single=True)
        dist, rs = pair_distances(T, pairs, c, single=True)
        live = dist * dist >= COINCIDENT2
        tied = np.nonzero(live & (np.abs(dist - rs) < tie))[0]
        sure = np.nonzero(live & (dist < rs) & (np.abs(dist - rs) >= tie))[0]
        n0 = 0 if sc.ground is None else int(((c[:, 2] - T.rad32 < sc.ground) & ((T.rad32 > 0) | (T.col_rim > 0))).sum())
        kept, count, over, rows = assemble(n0, list(sure), int(sc.n_lim[e]), sc.kmax)
        out.append(dict(sure=sure, tied=tied, coincident=int((~live).sum()), gap=float((dist - rs)[live].min()), n0=n0, kept=kept, over=over, rows=rows,
                        d_min=float(dist[sure].min()) if len(sure) else np.inf, coord=float(np.abs(c).max())))
    return pairs, out


def assert_the_designs_reach_the_edges(tie):
    """what the designed inputs must reach, asserted from the reference alone (tie: the tie band of whoever compares): the residues of n_self, more than 5 passes at
    16 lanes, hits at both ends of the list and on both sides of every pass boundary, several passes and two hits in one pass, coincident pairs, a dropped hit whose
    odd slot goes to a limit row, mixed lanes in every wave, gaps and overlaps >= 1e-4 m outside the grazing family, at most 1 % of the placements in the tie band"""
    comb, _, scenes = designed("A")
    n = len(comb.pairs)
    assert all(n % l != 0 for l in LANES) and 5 * 16 < n <= 30 * 16 and -(-n // 16) > 5 and comb.T.col_radius[0] > 0
    assert len(designed("B")[0].pairs) == 64
    cshape = designed("C")[0]
    assert (cshape.T.col_rim > 0).sum() == 2 and ((cshape.T.col_radius == 0) & (cshape.T.col_rim == 0)).sum() == 16
    assert not any(cshape.T.col_rim[s] > 0 for s in cshape.pairs.ravel()) and (cshape.T.col_radius[cshape.pairs].sum(axis=1) > 0).all()
    placements = tied_all = 0
    for which in "ABC":
        for name, sc in designed(which)[2].items():
            pairs, facts = scene_facts(sc, tie)
            placements += N_ENVS * len(pairs)
            tied_all += sum(len(f["tied"]) for f in facts)
            for e, f in enumerate(facts):
                assert f["coord"] <= 1.0 and f["d_min"] >= 0.05, (which, name, e)
                if not sc.label[e].startswith("grazing"):      # overlaps and gaps >= 1e-4 m: far outside the tie band
                    assert len(f["tied"]) == 0 and (len(f["sure"]) or f["gap"] >= 1e-4 - 1e-7), (which, name, e, sc.label[e], f["gap"])
            for lpe in LANES:      # every wave: at least a quarter of its envs hit nothing, and those that hit differ in which pairs
                per = 64 // lpe
                for w0 in range(0, N_ENVS, per):
                    hitting = [tuple(facts[e]["sure"]) for e in range(w0, w0 + per) if len(facts[e]["sure"])]
                    assert per == 1 or (per - len(hitting)) * 4 >= per and len(set(hitting)) == len(hitting), (which, name, lpe, w0)
            if (which, name) == ("A", "main"):
                hit = set(np.concatenate([f["sure"] for f in facts]).tolist())
                assert {0, n - 1} <= hit and all({l - 1, l} <= hit for l in LANES)
                multi = [f["sure"] for f in facts if len(f["sure"]) >= 2]
                for lpe in LANES:
                    assert any(len({p // lpe for p in s}) >= 3 for s in multi) and any(len({p // lpe for p in s}) == 2 for s in multi)
                    assert any(len(s) == 2 and s[0] // lpe == s[1] // lpe for s in multi)
                assert sum(f["coincident"] for f in facts) >= 4 and any(f["coincident"] and len(f["sure"]) for f in facts)
                assert sum(len(f["tied"]) for f in facts) >= 1      # the grazing family does use the exclusion
            if name.startswith("overflow"):
                assert [f["n0"] for f in facts[0:16:2]] == [c[0] for c in OVERFLOW_CASES[sc.kmax]] * 2
                assert any(f["over"] and f["rows"] == 1 and len(f["kept"]) < len(f["sure"]) and (sc.kmax - f["n0"]) % 2 == 1 for f in facts)      # dropped hit, odd slot to the limit row
                assert any(f["over"] and sc.n_lim[e] and f["rows"] == 0 for e, f in enumerate(facts))                                           # ... and a row without a slot
                assert any(not f["over"] and f["rows"] == 1 and f["n0"] + 2 * len(f["kept"]) + 1 == sc.kmax for f in facts)                       # last slot to the row, no overflow
    assert tied_all <= 0.01 * placements, (tied_all, placements)
