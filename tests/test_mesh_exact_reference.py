"""The mesh oracle (oracle/mesh_oracle.c) against an exact rational reference (mesh_exact_reference.py) on hard geometry
(mesh_geometry_cases.py).  The oracle and the HIP path are the same formulas, so their agreement says nothing about the
formulas themselves; this file pins the formulas.  CPU only; the device is held to the same reference in
test_gpu_mesh_geometry.py."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import mesh_exact_reference as X
import mesh_geometry_cases as G


# ---- the exact reference on cases computed by hand -------------------------------------------------------------------------
def _v(*p):
    return X.vec(p)


def test_exact_point_segment():
    a, b = _v(0, 0, 0), _v(2, 0, 0)
    assert X.point_segment_q(_v(1, 3, 4), a, b) == 25            # foot inside
    assert X.point_segment_q(_v(-3, 4, 0), a, b) == 25           # clamped to a
    assert X.point_segment_q(_v(5, 0, 4), a, b) == 25            # clamped to b
    assert X.point_segment_q(_v(1, 0, 0), a, b) == 0
    assert X.point_segment_q(_v(3, 4, 0), a, a) == 25            # a zero-length segment
    assert X.point_segment_q(_v(0.1, 0, 0), a, b) == 0 and X.point_segment_q(_v(0, 0.1, 0), a, b) == F(0.1) ** 2   # exact in the doubles given


def test_exact_point_triangle_in_every_region():
    A, B, C = _v(0, 0, 0), _v(4, 0, 0), _v(0, 4, 0)
    q = lambda *p: X.point_triangle_q(_v(*p), A, B, C)
    assert q(1, 1, 3) == 9 and q(1, 1, 0) == 0                   # face
    assert q(-3, -4, 0) == 25 and q(7, -4, 0) == 25 and q(-3, 8, 0) == 25      # the three vertex regions
    assert q(2, -3, 4) == 25 and q(-3, 2, 4) == 25               # edges AB, CA
    assert q(4, 4, 0) == 8 and q(4, 4, 1) == 9                   # edge BC: foot (2, 2, 0)
    assert q(0, 0, 0) == 0 and q(2, 2, 0) == 0 and q(2, 0, 0) == 0             # on the boundary
    # degenerate triangles fall back to their edges
    assert X.point_triangle_q(_v(1, 3, 0), A, B, _v(2, 0, 0)) == 9 and X.point_triangle_q(_v(3, 4, 0), A, A, A) == 25


def test_exact_segment_segment():
    q = lambda *c: X.segment_segment_q(_v(*c[0:3]), _v(*c[3:6]), _v(*c[6:9]), _v(*c[9:12]))
    assert q(-1, 0, 0, 1, 0, 0, 0, -1, 2, 0, 1, 2) == 4           # crossing in projection: the interior stationary point
    assert q(-1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0) == 0            # touching
    assert q(0, 0, 0, 1, 0, 0, 0, 3, 0, 1, 3, 0) == 9             # parallel
    assert q(0, 0, 0, 1, 0, 0, 3, 0, 0, 5, 0, 0) == 4             # collinear, disjoint
    assert q(0, 0, 0, 2, 0, 0, 1, 0, 0, 5, 0, 0) == 0             # collinear, overlapping
    assert q(0, 0, 0, 1, 0, 0, 4, 4, 0, 4, 8, 0) == 25            # end point to end point
    assert q(0, 0, 0, 0, 0, 0, 3, 4, 0, 3, 4, 0) == 25            # two points
    assert q(0, 0, 0, 4, 0, 0, 2, 1, -1, 2, 5, -1) == 2           # interior of one, end of the other


def test_exact_segment_triangle_and_mesh():
    A, B, C = _v(0, 0, 0), _v(4, 0, 0), _v(0, 4, 0)
    q = lambda *c: X.segment_triangle_q(_v(*c[0:3]), _v(*c[3:6]), A, B, C)
    assert q(1, 1, 1, 1, 1, -1) == 0                              # piercing
    assert q(1, 1, 1, 1, 1, 0) == 0 and q(2, 2, 5, 2, 2, 0) == 0  # ending on the face / on an edge
    assert q(0, 0, 3, 0, 0, 0) == 0                               # ending on a vertex
    assert q(3, 3, 1, 3, 3, -1) == 2                              # crossing the plane outside: distance to edge BC
    assert q(1, 1, 2, 2, 1, 3) == 4                               # above the face, end point closest
    assert q(0, 1, 3, 3, 1, 3) == 9                               # parallel above
    assert q(-1, -1, 0, 5, -1, 0) == 1                            # in the plane, outside
    assert q(-1, 1, 0, 5, 1, 0) == 0 and q(1, 1, 0, 2, 1, 0) == 0  # in the plane, across / inside
    assert q(-2, 6, 1, 6, -2, 1) == 1                             # over edge BC, both ends outside: the segment / edge pair
    tri = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 0, 2], [4, 0, 2], [0, 4, 2]]], float)
    assert X.mesh_q([1, 1, 3, 1, 2, 5], tri) == 1 and X.mesh_distance([1, 1, 0.5, 1, 2, 0.5], tri) == 0.5
    assert X.triangle_min_altitude(tri[0]) == math.sqrt(8.0) and X.triangle_min_altitude(np.zeros((3, 3))) == 0.0


def test_exact_reference_is_invariant_under_relabelling():
    """the minimum over faces must not depend on the order of the vertices or on the direction of the segment -- exactly"""
    rng = np.random.default_rng(5)
    for _ in range(25):
        T, s = rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, 6)
        q = X.mesh_q(s, T[None])
        assert q == X.mesh_q(s, T[[1, 2, 0]][None]) == X.mesh_q(s, T[[2, 1, 0]][None]) == X.mesh_q(s[[3, 4, 5, 0, 1, 2]], T[None])


# ---- the oracle against the exact reference -----------------------------------------------------------------------------
def _oracle_errors(O, name):
    """per case of the family: (tri, segs, exact, |oracle - exact|)"""
    out = []
    for (tri, segs), ex in zip(G.family(name).cases, G.exact(name)):
        O.mesh_register(11, tri)
        od = O.mesh_seg_distance(11, segs)[0]
        out.append((tri, segs, ex, np.abs(od - ex)))
    return out


@pytest.mark.parametrize("name", G.NAMES["far"] + G.NAMES["lattice"])
def test_oracle_against_exact_away_from_contact(O, name):
    worst = 0.0
    for tri, segs, ex, err in _oracle_errors(O, name):
        if name != "lattice":
            assert ex.min() >= G.FAR_MIN
        L = np.array([G.coord_scale(tri, s) for s in segs])
        worst = max(worst, float((err / L).max()))
        assert np.all(err <= 16 * G.EPS * L), (name, float((err / (G.EPS * L)).max()))
    print(f"{name}: worst oracle error {worst / G.EPS:.2f} eps L")


def test_lattice_family_has_contacts_and_gaps(O):
    ex = np.concatenate(G.exact("lattice"))
    assert (ex == 0).sum() > 40 and (ex == 0.25).sum() > 10 and (ex > 0).sum() > 40


@pytest.mark.parametrize("name", G.NAMES["contact"])
def test_oracle_against_exact_near_contact(O, name):
    """Only the derivable part is asserted: a crossing decided the other way costs at most the way from a point of the
    triangle to its boundary, which is below the smallest altitude.  Zero against non-zero is not asserted at offsets 0 and
    1e-15.  The worst error is printed, and held to what CONTACT_ORACLE_ERR records (the measurement rounded up to two
    digits): the device's bound is derived from that table, so it must not go stale."""
    worst = 0.0
    for tri, segs, ex, err in _oracle_errors(O, name):
        L = np.array([G.coord_scale(tri, s) for s in segs])
        alt = X.triangle_min_altitude(tri[0])
        assert ex.max() < 2e-9                                      # the family is at contact: nothing further than the largest offset
        assert np.all(err <= alt + 16 * G.EPS * L), (name, float(err.max()), alt)
        worst = max(worst, float(err.max()))
    print(f"{name}: worst oracle error {worst:.3e} m (recorded: {G.CONTACT_ORACLE_ERR[name]:.1e})")
    assert worst <= G.CONTACT_ORACLE_ERR[name]


# ---- the traversal family is what its docstring says (the GPU test relies on it) ------------------------------------------------
def test_traversal_family_shapes(O):
    cases = G.family("traversal").cases
    nts = [c[0].shape[0] for c in cases]
    assert nts[:4] == [2048, 2048, 64, 2248] and nts[4:19] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 129]
    assert [c[1].shape[0] for c in cases[19:]] == [1, 127, 128, 129] and 1400 <= cases[0][1].shape[0] <= 1600
    wall = cases[0][0]
    assert np.ptp(wall[..., 0]) == 0.0                               # zero thickness
    verts, counts = np.unique(wall.reshape(-1, 3), axis=0, return_counts=True)
    assert verts.shape[0] == 33 * 33 and (counts == 6).sum() == 31 * 31      # shared vertices are bitwise equal
    # the queries touch, cross and miss: the oracle sees exact zeros, exact ties at 1e-3 / 0.3 and far misses
    O.mesh_register(11, wall)
    d = O.mesh_seg_distance(11, cases[0][1])[0]
    assert (d == 0).sum() > 300 and (np.abs(d - 0.3) < 1e-15).sum() > 50 and (np.abs(d - 1e-3) < 1e-15).sum() > 50 and d.max() > 0.5
