"""Pins tests/ray_bodies_reference.py, the fp64 reference the GPU tests of rsb_ray_cast / rsb_ray_scan judge the device by: the entry parameters
of rays in closed form, the signed distances against a brute-force search over sampled surfaces, and the shapes read from the ANYmal-like model."""
import numpy as np
import pytest

import ray_bodies_reference as rb
from raisimlib_amd import Model, rsc_path

R3, R2 = np.sqrt(3.0), np.sqrt(2.0)
Q = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])      # a rotation (rows orthonormal, det +1)
SPHERE = dict(kind="sphere", body=0, prim=0, centre=np.array([0.3, -0.2, 0.5]), radius=0.25)
CAPSULE = dict(kind="capsule", body=0, prim=1, a=np.array([0.0, 0.0, 0.2]), b=np.array([0.0, 0.0, -0.4]), radius=0.1)
CYLINDER = dict(kind="cylinder", body=0, prim=3, a=np.array([0.0, 0.0, 0.2]), b=np.array([0.0, 0.0, -0.4]), radius=0.1)
BOX = dict(kind="box", body=0, prim=5, centre=np.zeros(3), half=np.diag([0.2, 0.2, 0.2]))
SLAB = dict(kind="box", body=0, prim=5, centre=np.array([0.1, 0.2, -0.3]), half=np.diag([0.3, 0.1, 0.05]) @ Q)      # tilted, three different edges
TILTED_CAPSULE = dict(CAPSULE, a=Q.T @ CAPSULE["a"] + 0.1, b=Q.T @ CAPSULE["b"] + 0.1)
TILTED_CYLINDER = dict(CYLINDER, a=Q.T @ CYLINDER["a"] - 0.2, b=Q.T @ CYLINDER["b"] - 0.2)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def test_entry_parameters_in_closed_form():
    near = lambda a, b: abs(a - b) <= 1e-12      # noqa: E731
    c = SPHERE["centre"]
    d = unit([1.0, 2.0, -0.5])
    assert near(rb.first_entry(SPHERE, c - 3.0 * d, d, 10.0), 3.0 - 0.25)      # through the centre
    assert rb.first_entry(SPHERE, c - 3.0 * d, d, 2.0) is None and rb.first_entry(SPHERE, c + 3.0 * d, d, 10.0) is None      # too far, behind
    assert rb.first_entry(SPHERE, c + [0.26, 0, 0], unit([0, 1, 0]), 10.0) is None      # past it
    assert near(rb.first_entry(SPHERE, c + [0.1, 0.0, 2.0], [0, 0, -1.0], 10.0), 2.0 - np.sqrt(0.25 ** 2 - 0.1 ** 2))      # off centre
    z = np.array([0.0, 0.0, 1.0])
    assert near(rb.first_entry(CAPSULE, [0, 0, 2.0], -z, 10.0), 2.0 - 0.2 - 0.1)      # along the axis: the end sphere
    assert near(rb.first_entry(CAPSULE, [0, 0, -2.0], z, 10.0), 2.0 - 0.4 - 0.1)
    assert near(rb.first_entry(CAPSULE, [1.0, 0, -0.1], [-1.0, 0, 0], 10.0), 0.9)      # across the barrel
    assert near(rb.first_entry(CAPSULE, [1.0, 0, 0.25], [-1.0, 0, 0], 10.0), 1.0 - np.sqrt(0.1 ** 2 - 0.05 ** 2))      # across the end sphere
    assert rb.first_entry(CAPSULE, [1.0, 0, 0.31], [-1.0, 0, 0], 10.0) is None
    assert near(rb.first_entry(CYLINDER, [0.05, 0, 2.0], -z, 10.0), 1.8)       # onto the cap
    assert near(rb.first_entry(CYLINDER, [1.0, 0, -0.1], [-1.0, 0, 0], 10.0), 0.9)      # onto the barrel
    assert rb.first_entry(CYLINDER, [1.0, 0, 0.21], [-1.0, 0, 0], 10.0) is None      # over the flat cap, where the capsule is still round
    assert near(rb.first_entry(CYLINDER, [0.3, 0, 0.5], unit([-1.0, 0, -1.0]), 10.0), 0.3 * R2)      # the cap, reached obliquely at radius 0
    assert near(rb.first_entry(BOX, [0.1, -0.05, 3.0], -z, 10.0), 2.8)         # a face
    assert near(rb.first_entry(BOX, [3.0, 3.0, 0.1], unit([-1.0, -1.0, 0]), 10.0), 2.8 * R2)      # an edge
    assert near(rb.first_entry(BOX, [3.0, 3.0, 3.0], unit([-1.0, -1.0, -1.0]), 10.0), 2.8 * R3)   # a corner
    assert rb.first_entry(BOX, [3.0, 3.0, 0.1], unit([-1.0, -1.0 - 1e-3, 0]), 10.0) is not None and rb.first_entry(BOX, [3.0, 3.0, 0.1], unit([-1.0, -0.8, 0]), 10.0) is None
    # the tilted box is the axis-aligned one seen from a turned frame
    o, dd = np.array([0.7, -0.1, 0.4]), unit([-1.0, 0.3, -0.6])
    straight = dict(SLAB, centre=np.zeros(3), half=np.diag([0.3, 0.1, 0.05]))
    a, b = rb.interval(SLAB, o, dd), rb.interval(straight, Q @ (o - SLAB["centre"]), Q @ dd)
    assert (a is None) == (b is None)
    o = SLAB["centre"] + Q.T @ np.array([0.1, 0.02, 1.0])
    assert near(rb.first_entry(SLAB, o, -Q.T @ z, 10.0), 0.95)
    # origins inside
    for s, inside in ((SPHERE, c + [0.1, 0.1, 0.0]), (CAPSULE, [0.05, 0, 0.25]), (CYLINDER, [0.05, 0, 0.15]), (BOX, [0.1, -0.1, 0.15]), (SLAB, SLAB["centre"])):
        for d in (z, -z, unit([1, 1, 1])):
            assert rb.first_entry(s, np.asarray(inside, float), d, 10.0) == 0.0
            assert rb.phi(s, np.asarray(inside, float)) < 0


def surface_points(shape, n=120):
    """points on the surface of a shape, no further apart than about its size / n * 3"""
    kind = shape["kind"]
    u, v = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    u, v = u.ravel(), v.ravel()
    ball = lambda c, r: c + r * np.stack([np.sin(np.pi * u) * np.cos(2 * np.pi * v), np.sin(np.pi * u) * np.sin(2 * np.pi * v), np.cos(np.pi * u)], axis=-1)      # noqa: E731
    if kind == "sphere":
        return ball(shape["centre"], shape["radius"])
    if kind == "box":
        pts = []
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            for sgn in (-1.0, 1.0):
                pts.append(shape["centre"] + sgn * shape["half"][k] + np.outer(2 * u - 1, shape["half"][i]) + np.outer(2 * v - 1, shape["half"][j]))
        return np.concatenate(pts)
    a, b, r = shape["a"], shape["b"], shape["radius"]
    n_ax = (b - a) / np.linalg.norm(b - a)
    e1 = unit(np.cross(n_ax, [1.0, 0.3, 0.2]))
    e2 = np.cross(n_ax, e1)
    ring = np.outer(np.cos(2 * np.pi * v), e1) + np.outer(np.sin(2 * np.pi * v), e2)
    barrel = a + np.outer(u, b - a) + r * ring
    if kind == "capsule":
        cap_a, cap_b = ball(a, r), ball(b, r)      # the outer halves of the end spheres
        return np.concatenate([barrel, cap_a[(cap_a - a) @ n_ax <= 0], cap_b[(cap_b - b) @ n_ax >= 0]])
    return np.concatenate([barrel, a + (r * u)[:, None] * ring, b + (r * u)[:, None] * ring])


@pytest.mark.parametrize("shape", [SPHERE, TILTED_CAPSULE, TILTED_CYLINDER, SLAB], ids=lambda s: s["kind"])
def test_signed_distance_against_sampled_surfaces(shape):
    pts = surface_points(shape)
    assert np.abs(rb.phi(shape, pts)).max() <= 1e-12      # the samples lie on the surface
    rng = np.random.default_rng(1)
    centre = pts.mean(axis=0)
    x = centre + np.concatenate([rng.uniform(-0.7, 0.7, (200, 3)), rng.uniform(-0.15, 0.15, (100, 3))])[rng.permutation(300)]      # far and near
    brute = np.array([np.linalg.norm(pts - p, axis=1).min() for p in x])
    got = rb.phi(shape, x)
    assert (got < 0).sum() >= 5 and (got > 0).sum() >= 100
    # the nearest sample is at most half a sample spacing (size / 120 * pi) off the nearest surface point
    assert np.all(brute >= np.abs(got) - 1e-12) and np.all(brute <= np.abs(got) + 0.02)
    # the sign: inside means every ray leaves through the surface, outside that some ray never meets it
    for p, g in zip(x[:60], got[:60]):
        away = unit(p - centre)
        assert (rb.first_entry(shape, p, away, 50.0) == 0.0) == (g <= 0)


def test_shapes_of_the_anymal_like_model():
    m = Model(urdf_path=rsc_path("anymal_c_like.urdf"))
    shapes = rb.shapes_of(m.blob)
    name = lambda s: bytes(m.blob.body_name[s["body"]]).split(b"\0")[0].decode()      # noqa: E731
    col = lambda s: bytes(m.blob.col_name[s["prim"]]).split(b"\0")[0].decode()         # noqa: E731
    spheres = [s for s in shapes if s["kind"] == "sphere"]
    capsules = [s for s in shapes if s["kind"] == "capsule"]
    assert len(shapes) == 16 and len(spheres) == 12 and len(capsules) == 4
    assert [name(s) for s in spheres if col(s).startswith("base")] == ["base"] * 4
    legs = ("LF", "RF", "LH", "RH")
    assert sorted(name(s) for s in spheres if col(s).endswith("_knee")) == sorted(leg + "_SHANK" for leg in legs)
    assert sorted(name(s) for s in spheres if col(s).endswith("_foot")) == sorted(leg + "_SHANK" for leg in legs)
    assert sorted(name(s) for s in capsules) == sorted(leg + "_THIGH" for leg in legs)
    for s in capsules:      # the capsule swallows both of its end primitives
        assert int(m.blob.col_capsule[s["prim"]]) == s["prim"] + 2 and s["radius"] == 0.045 and np.linalg.norm(s["a"] - s["b"]) > 0.1
    assert [s["prim"] for s in shapes] == sorted(s["prim"] for s in shapes)
    # a pose moves a shape rigidly
    R, p = Q.T, np.array([1.0, 2.0, 3.0])
    w = rb.to_world(capsules[0], [(R, p)] * m.nb)
    assert np.allclose(w["a"], p + R @ capsules[0]["a"]) and np.isclose(np.linalg.norm(w["a"] - w["b"]), np.linalg.norm(capsules[0]["a"] - capsules[0]["b"]))
