"""Exact segment / triangle / mesh distances in rational arithmetic: the ground truth of the mesh tests.

oracle/mesh_oracle.c and csrc/cfs_mesh_dev.h are the same formulas (Voronoi-region walk, piercing predicate, distLinSeg), so
a wrong region test would be wrong on both sides.  This module shares nothing with them: a distance is the minimum of a convex
quadratic over a product of simplices, and such a minimum is attained either at an interior stationary point or on a face, so
it is written as "the minimum over the faces, plus the interior candidate where it exists".  Every number is a
fractions.Fraction of the doubles as given (Fraction(float) is exact), every predicate is therefore decided exactly, and the
functions return the exact SQUARED distance; `dist` takes the one square root at the end.
"""
import math
from fractions import Fraction

ZERO, ONE = Fraction(0), Fraction(1)


def vec(p):
    """three doubles -> three exact rationals"""
    return (Fraction(float(p[0])), Fraction(float(p[1])), Fraction(float(p[2])))


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _along(a, d, t):
    return (a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2])


def point_segment_q(p, a, b):
    """|p - [a, b]|^2: the projection on the line, clamped to the segment"""
    d = _sub(b, a)
    D = _dot(d, d)
    ap = _sub(p, a)
    if D == 0:
        return _dot(ap, ap)
    t = min(ONE, max(ZERO, _dot(ap, d) / D))
    e = _sub(ap, (t * d[0], t * d[1], t * d[2]))
    return _dot(e, e)


def _barycentric_inside(x, A, ab, ac, n, nn):
    """is the projection of x on the plane of the (proper) triangle in the closed triangle?  x - A = beta ab + gamma ac + lambda n"""
    ax = _sub(x, A)
    beta = _dot(_cross(ax, ac), n)          # times nn > 0: only the signs matter
    gamma = _dot(_cross(ab, ax), n)
    return beta >= 0 and gamma >= 0 and beta + gamma <= nn


def point_triangle_q(p, A, B, C):
    """|p - ABC|^2: the three edges, and the plane where the projection falls in the closed triangle"""
    q = min(point_segment_q(p, A, B), point_segment_q(p, B, C), point_segment_q(p, C, A))
    ab, ac = _sub(B, A), _sub(C, A)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    if nn != 0 and _barycentric_inside(p, A, ab, ac, n, nn):
        h = _dot(_sub(p, A), n)
        q = min(q, h * h / nn)
    return q


def segment_segment_q(p0, p1, q0, q1):
    """|[p0, p1] - [q0, q1]|^2: the four end points against the other segment, and the stationary point of the quadratic in
    (s, t) where it is unique and lies in the closed unit square"""
    q = min(point_segment_q(p0, q0, q1), point_segment_q(p1, q0, q1), point_segment_q(q0, p0, p1), point_segment_q(q1, p0, p1))
    d1, d2, r = _sub(p1, p0), _sub(q1, q0), _sub(p0, q0)
    D1, D2, R = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2)
    den = D1 * D2 - R * R
    if den != 0:
        c, f = _dot(d1, r), _dot(d2, r)
        s, t = (R * f - c * D2) / den, (D1 * f - R * c) / den      # gradient of |r + s d1 - t d2|^2 = 0
        if 0 <= s <= 1 and 0 <= t <= 1:
            e = _sub(_along(r, d1, s), (t * d2[0], t * d2[1], t * d2[2]))
            q = min(q, _dot(e, e))
    return q


def segment_triangle_q(p0, p1, A, B, C):
    """|[p0, p1] - ABC|^2: 0 when the segment crosses the plane of a proper triangle inside the closed triangle, otherwise the
    two end points against the triangle and the segment against the three edges (a segment in the plane of the triangle that
    meets it either crosses an edge or has an end point inside: both are among those)"""
    ab, ac = _sub(B, A), _sub(C, A)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    if nn != 0:
        s0, s1 = _dot(n, _sub(p0, A)), _dot(n, _sub(p1, A))
        if s0 != s1 and s0 * s1 <= 0:
            x = _along(p0, _sub(p1, p0), s0 / (s0 - s1))
            if _barycentric_inside(x, A, ab, ac, n, nn):
                return ZERO
    return min(point_triangle_q(p0, A, B, C), point_triangle_q(p1, A, B, C),
               segment_segment_q(p0, p1, A, B), segment_segment_q(p0, p1, B, C), segment_segment_q(p0, p1, C, A))


def mesh_q(seg, tri):
    """exact squared distance of the segment seg (6 doubles) to the triangles tri (nt, 3, 3): the minimum over the triangles"""
    p0, p1 = vec(seg[:3]), vec(seg[3:6])
    return min(segment_triangle_q(p0, p1, vec(T[0]), vec(T[1]), vec(T[2])) for T in tri)


def dist(q):
    """the one rounding step: exact squared distance -> double.  float(Fraction) rounds correctly, so the result is within
    1 ulp of the true distance."""
    return math.sqrt(float(q))


def mesh_distance(seg, tri):
    return dist(mesh_q(seg, tri))


def triangle_min_altitude(T):
    """smallest altitude of the triangle T (3, 3) as a double (0 for a degenerate one): how far a point of the triangle can be
    from its boundary at most, i.e. the most a misclassified crossing can cost"""
    A, B, C = vec(T[0]), vec(T[1]), vec(T[2])
    n = _cross(_sub(B, A), _sub(C, A))
    nn = _dot(n, n)
    if nn == 0:
        return 0.0
    longest = max(_dot(_sub(B, A), _sub(B, A)), _dot(_sub(C, B), _sub(C, B)), _dot(_sub(A, C), _sub(A, C)))
    return math.sqrt(float(nn / longest))
