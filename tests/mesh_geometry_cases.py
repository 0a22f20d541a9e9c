"""Seeded hard-geometry cases for the mesh distance queries, shared by the CPU tests (oracle against the exact reference:
test_mesh_exact_reference.py) and the GPU tests (device against both: test_gpu_mesh_geometry.py).

A family is a list of cases (tri (nt, 3, 3), segs (n, 6)) under a name, with a kind that says what is asserted about it:

  far        exact distance >= FAR_MIN (kept by the exact reference, not hand-picked): generic triangles, slivers
             C = A + s (B - A) + eps noise with eps = 1e-3 .. 1e-15, needles with two vertices eps apart and exactly degenerate
             triangles (collinear, two vertices equal, all three equal), each in three placements: coordinates in [-2, 2]; the
             shape scaled by 0.01 at the cell offset (3.6, 8.4, 0.5); the shape scaled by 0.01 at an offset of 1e3.  In the two
             scaled placements the segments stay arm-sized (a box of half-width 0.5 around the shape).
             Bound: 16 eps L (forward error of well-conditioned fp64 formulas of this depth), L the largest |coordinate|.
  lattice    every coordinate a multiple of 1/4, so that every predicate of the fp64 formulas is exact: in-plane, parallel,
             collinear-overlapping, vertex-touching, edge-ending and zero-length segments.  Bound: 16 eps L.
  contact    segments aimed at a point of the triangle (interior, edge, vertex: passing the point at a lateral offset; "end":
             stopping short of an interior point by the offset) with offsets 0, 1e-15 and 1e-9.  The predicates are
             ill-conditioned here, so no tolerance is fixed in advance: the derivable bound is the triangle's smallest altitude
             (a misclassified crossing costs at most that) + 16 eps L, and the oracle's worst error against the exact
             reference, measured on the CPU (gcc -O2, x86-64, no FMA contraction), is recorded per family in
             CONTACT_ORACLE_ERR:

                 contact_generic        3.0e-16 m
                 contact_sliver_1e-4    8.4e-9 m
                 contact_sliver_1e-8    7.7e-9 m
                 contact_sliver_1e-12   4.3e-13 m

             The 1e-8 m on the 1e-4 slivers is not a misclassified crossing: it is the face branch of the Voronoi-region walk.
             Its barycentric weights are quotients by |n|^2 = |AB x AC|^2, so the foot point moves along the sliver by about
             eps / sin^2 of the sliver's angle; an end point 1e-9 above the face then measures its distance to a foot point 1e-8
             to the side.  The result stays a point of the triangle (the weights are positive), so the error is one-sided and
             below the altitude, and it vanishes quadratically with the distance (nothing of it is left in the far families).

             Both device builds of the query are held to 4x these figures (FMA contraction re-rounds the same predicates),
             floor 1e-12; test_mesh_exact_reference.py holds the oracle to the figures themselves.
  traversal  meshes, compared with the brute-force oracle: a flat axis-aligned 32 x 32 grid wall (every box has zero thickness,
             every inner vertex is shared by six triangles), the same wall tilted by an irrational angle, one triangle repeated
             64 times (all centroids equal), a wall plus 200 slivers, random soups of 1..9, 63, 64, 65, 127, 128, 129
             triangles (leaf boundaries for two triangles per leaf); query counts of 1, 127, 128, 129 and about 1 500.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import mesh_exact_reference as X

EPS = 2.2e-16
FAR_MIN = 1e-2
CELL = np.array([3.6, 8.4, 0.5])
OFFSETS = (0.0, 1e-15, 1e-9)

# worst |oracle - exact| per contact family, metres (measured by test_mesh_exact_reference.py::test_contact_...; see above)
CONTACT_ORACLE_ERR = {
    "contact_generic": 3.0e-16,
    "contact_sliver_1e-4": 8.4e-9,
    "contact_sliver_1e-8": 7.7e-9,
    "contact_sliver_1e-12": 4.3e-13,
}

Family = namedtuple("Family", "name kind cases")          # cases: list of (tri (nt, 3, 3), segs (n, 6))


def coord_scale(tri, seg):
    """L of the bound 16 eps L: the largest absolute coordinate of the pair"""
    return max(float(np.abs(tri).max()), float(np.abs(seg).max()))


# ---- shapes ----------------------------------------------------------------------------------------------------------
def _generic(rng, n):
    return [rng.uniform(-1, 1, (3, 3)) for _ in range(n)]


def _sliver(rng, eps):
    A, B = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    return np.stack([A, B, A + rng.uniform(0.2, 0.8) * (B - A) + eps * rng.standard_normal(3)])


def _needle(rng, eps):
    A, C = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    return np.stack([A, A + eps * rng.standard_normal(3), C])


def _degenerate(rng):
    A, B = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    A, B = np.round(A * 64) / 64, np.round(B * 64) / 64            # A + (B - A) / 4 is then exactly on the line
    return [np.stack([A, B, A + 0.25 * (B - A)]), np.stack([A, B, A + 1.5 * (B - A)]),    # collinear: C inside AB, C beyond B
            np.stack([A, A, B]), np.stack([A, B, B]), np.stack([A, B, A]), np.stack([A, A, A])]


def _far_shapes(rng):
    eps = (1e-3, 1e-6, 1e-9, 1e-12, 1e-15)
    deg = _degenerate(rng)
    assert all(X.triangle_min_altitude(T) == 0.0 for T in deg)     # exactly degenerate, not nearly
    return {"generic": _generic(rng, 5),
            "sliver": [_sliver(rng, e) for e in eps],
            "needle": [_needle(rng, e) for e in eps],
            "degenerate": deg}


def _far_family(name, shapes, place, rng, per_shape):
    cases = []
    for T in shapes:
        if place == "unit":
            tri, a = T, rng.uniform(-2, 2, (4 * per_shape, 3))
            b = (a + rng.normal(0, 0.7, a.shape)).clip(-2, 2)
        else:
            off = CELL if place == "cell" else np.full(3, 1e3)
            tri = 0.01 * T + off
            a = off + rng.uniform(-0.5, 0.5, (4 * per_shape, 3))
            b = a + rng.normal(0, 0.25, a.shape)
        segs = np.concatenate([a, b], axis=1)
        segs[::7, 3:] = segs[::7, :3]                                # some zero-length segments
        keep = []
        for s in segs:                                               # the first per_shape that the exact reference calls far
            if len(keep) < per_shape and X.mesh_q(s, tri[None]) >= X.Fraction(FAR_MIN) ** 2:
                keep.append(s)
        assert len(keep) == per_shape, (name, len(keep))
        cases.append((tri[None], np.array(keep)))
    return Family(name, "far", cases)


# ---- lattice -----------------------------------------------------------------------------------------------------------
def _lattice_family():
    T0 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    T1 = np.array([[1.0, 0, 0], [1, 1, 0.5], [0, 1, 0]])                # shares the hypotenuse of T0
    q = 0.25
    segs = [
        # in the plane z = 0: inside, across an edge, outside and parallel to an edge, outside towards a vertex
        [q, q, 0, 2 * q, q, 0], [q, q, 0, 1.5, q, 0], [-1, -q, 0, 2, -q, 0], [-1, -1, 0, -q, -q, 0], [2, 0, 0, 1.25, 0, 0],
        [q, -1, 0, q, 2, 0], [-q, 1.25, 0, 1.25, -q, 0],
        # parallel to the plane at z = 1/4: over the inside, over an edge, outside
        [q, q, q, 2 * q, 2 * q, q], [0, 0, q, 1, 0, q], [-1, -q, q, 2, -q, q], [-2, -2, q, -1, -1, q], [0, 0.5, q, 0.5, 0, q],
        # collinear with an edge and overlapping it: partly, wholly, containing it, disjoint on the same line
        [0.5, 0, 0, 1.5, 0, 0], [q, 0, 0, 3 * q, 0, 0], [-1, 0, 0, 2, 0, 0], [1.25, 0, 0, 2, 0, 0], [0, q, 0, 0, 3 * q, 0],
        [1.25, -q, 0, -q, 1.25, 0], [3 * q, q, 0, q, 3 * q, 0],
        # touching a vertex: from above, in the plane, passing through
        [0, 0, 1, 0, 0, 0], [-1, -1, 0, 0, 0, 0], [1, 0, 1, 1, 0, -1], [0, 1, 0, 0, 2, 1], [-1, 1, 0, 1, -1, 0],
        # ending on an edge, from above and in the plane; ending inside
        [0.5, 0, 1, 0.5, 0, 0], [0.5, -1, 0, 0.5, 0, 0], [0.5, 0.5, 0.75, 0.5, 0.5, 0], [q, q, 1, q, q, 0],
        # piercing: inside, through an edge, through the shared edge, missing
        [q, q, 1, q, q, -1], [0.5, 0, 1, 0.5, 0, -1], [0.5, 0.5, 1, 0.5, 0.5, -1], [1, 1, 1, 1, 1, -1], [0.75, 0.75, 1, 0.75, 0.75, -1],
        # zero length: at a vertex, on an edge, inside, above, outside
        [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 0], [0.5, 0, 0, 0.5, 0, 0], [0.5, 0.5, 0, 0.5, 0.5, 0], [q, q, 0, q, q, 0],
        [q, q, 0.5, q, q, 0.5], [2, 2, 0, 2, 2, 0], [1, 1, 0.5, 1, 1, 0.5],
    ]
    segs = np.array(segs, float)
    both = np.concatenate([segs, segs[:, [3, 4, 5, 0, 1, 2]]])          # and every segment reversed
    assert np.all(both * 4 == np.round(both * 4))
    return Family("lattice", "lattice", [(T0[None], both), (T1[None], both), (np.stack([T0, T1]), both), (np.stack([T1, T0]), both)])


# ---- contact -------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def _contact_family(name, tris, rng, ndir):
    cases = []
    for T in tris:
        A, B, C = T
        n = np.cross(B - A, C - A)
        n = _unit(n) if np.linalg.norm(n) > 0 else _unit(np.cross(B - A, [0.3, -0.5, 0.8]))
        segs = []
        for _ in range(ndir):
            w = rng.dirichlet([2, 2, 2])
            s = rng.uniform(0.1, 0.9)
            out_ab = _unit(np.cross(B - A, n))                          # in the plane, across AB
            if np.dot(out_ab, C - A) > 0:
                out_ab = -out_ab                                        # pointing away from the triangle
            targets = {"interior": (w[0] * A + w[1] * B + w[2] * C, out_ab),
                       "edge": (A + s * (B - A), out_ab),
                       "vertex": (A, _unit(A - (B + C) / 2)),
                       "end": (w[0] * A + w[1] * B + w[2] * C, None)}
            u = _unit(n * rng.choice([-1, 1]) * rng.uniform(0.3, 1.0) + 0.6 * rng.standard_normal(3))   # approach direction, off the plane
            for kind, (P, lateral) in targets.items():
                for off in OFFSETS:
                    start = P + rng.uniform(0.2, 0.6) * u
                    if kind == "end":                                   # stops short of the surface by `off`
                        segs.append(np.concatenate([start, P + off * u]))
                    else:                                               # goes through, passing the target at a lateral distance `off`
                        segs.append(np.concatenate([start + off * lateral, P - rng.uniform(0.2, 0.6) * u + off * lateral]))
        cases.append((T[None], np.array(segs)))
    assert sum(c[1].shape[0] for c in cases) <= 400
    return Family(name, "contact", cases)


# ---- traversal -------------------------------------------------------------------------------------------------------------
def grid_wall(p0, du, dv, n=32):
    """n x n quads on the parallelogram p0 + s du + t dv, two triangles each; a shared vertex is one double triple"""
    p0, du, dv = np.asarray(p0, float), np.asarray(du, float), np.asarray(dv, float)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    P = p0 + (i / n)[..., None] * du + (j / n)[..., None] * dv
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    return np.concatenate([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)])


def _rotation(angle, axis):
    k = _unit(np.asarray(axis, float))
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def mesh_queries(tri, normal, rng, per):
    """the query families of one mesh, `per` of each: on the faces of the bounding box and along triangle edges / between
    vertices (grid lines of a wall), those moved off the surface by 1e-3 and 0.3 along `normal`, across the whole bounding
    box, ten times longer than the mesh, zero length at vertices, end points exactly on slab boundaries (coordinates of
    vertices and of the bounding box, which are the faces of the hierarchy's boxes)"""
    V = tri.reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    ext = np.maximum(hi - lo, 0.05)
    diag = np.linalg.norm(ext)
    normal = np.asarray(normal, float)
    out = []

    def pick(k):
        return V[rng.integers(0, V.shape[0], k)]

    # along triangle edges and between vertices (in the plane of a wall: along and across its grid lines)
    t = tri[rng.integers(0, tri.shape[0], per)]
    edges = np.concatenate([t[:, 0], t[:, 1]], axis=1)
    between = np.concatenate([pick(per), pick(per)], axis=1)
    out += [edges, between]
    # on the faces of the bounding box
    a, b = rng.uniform(lo, lo + ext, (per, 3)), rng.uniform(lo, lo + ext, (per, 3))
    ax, side = rng.integers(0, 3, per), rng.integers(0, 2, per)
    for k in range(per):
        a[k, ax[k]] = b[k, ax[k]] = (lo, hi)[side[k]][ax[k]]
    out.append(np.concatenate([a, b], axis=1))
    # parallel to the surface at 1e-3 and at 0.3
    for h in (1e-3, 0.3):
        sgn = rng.choice([-1.0, 1.0], (per, 1))
        sh = h * sgn * normal
        out.append(np.concatenate([between[:, :3] + sh, between[:, 3:] + sh], axis=1))
    # across the whole bounding box, and ten times longer than the mesh
    c = rng.uniform(lo, lo + ext, (per, 3))
    u = rng.standard_normal((per, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out.append(np.concatenate([c - 1.1 * diag * u, c + 1.1 * diag * u], axis=1))
    c2 = c + 0.3 * diag * rng.standard_normal((per, 3))
    out.append(np.concatenate([c2 - 5 * diag * u, c2 + 5 * diag * u], axis=1))
    # zero length at vertices
    v = pick(per)
    out.append(np.concatenate([v, v], axis=1))
    # end points exactly on slab boundaries: each coordinate that of some vertex or of the bounding box, one end pushed outside
    p = np.stack([pick(per)[:, 0], pick(per)[:, 1], pick(per)[:, 2]], axis=1)
    q = np.stack([pick(per)[:, 0], pick(per)[:, 1], pick(per)[:, 2]], axis=1)
    q[::2] = np.where(rng.integers(0, 2, (len(q[::2]), 3)) == 0, lo, hi)
    r = q.copy()
    r[np.arange(per), ax] += side * 2 * diag - diag                    # leaves the box along one axis, the other two stay on boundaries
    out += [np.concatenate([p, q], axis=1), np.concatenate([q, r], axis=1)]
    return np.concatenate(out)


def _traversal_family():
    rng = np.random.default_rng(2025)
    wall = flat_wall()
    Rm = _rotation(1.0, [1.0, 2.0, 3.0])                                 # 1 rad: no multiple of pi
    centre = wall.reshape(-1, 3).mean(0)
    tilted = (wall - centre) @ Rm.T + centre
    nx, nt_ = np.array([1.0, 0, 0]), Rm @ np.array([1.0, 0, 0])
    one = rng.uniform(-1, 1, (3, 3))
    cases = [("wall", wall, nx, 140), ("tilted", tilted, nt_, 140), ("repeated", np.repeat(one[None], 64, axis=0), np.array([0, 0, 1.0]), 30),
             ("sliver_wall", sliver_wall(), nx, 140)]
    for nt in (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 129):
        cases.append((f"soup{nt}", rng.uniform(-1, 1, (nt, 3, 3)), np.array([0, 0, 1.0]), 30))
    out = []
    for name, tri, normal, per in cases:
        out.append((tri, mesh_queries(tri, normal, rng, per)))
    q = mesh_queries(wall, nx, rng, 140)
    q = q[rng.permutation(q.shape[0])]
    for n in (1, 127, 128, 129):                                         # ragged against the 128-thread block
        out.append((wall, q[:n]))
    return Family("traversal", "traversal", out)


WALL = ([3.9, 8.0, 0.1], [0, 0.8, 0], [0, 0, 0.8])                      # the plane x = 3.9 in the cell; du x dv = +x


def flat_wall(p0=WALL[0], du=WALL[1], dv=WALL[2]):
    return grid_wall(p0, du, dv)


def sliver_wall(p0=WALL[0], du=WALL[1], dv=WALL[2]):
    """the flat wall plus 200 slivers (1e-4 .. 1e-12 wide) standing on the side du x dv points away from, up to 0.1 in front
    of the wall, some sticking through it"""
    rng = np.random.default_rng(77)
    p0, du, dv = np.asarray(p0, float), np.asarray(du, float), np.asarray(dv, float)
    n = _unit(np.cross(du, dv))
    sl = []
    for k in range(200):
        A = p0 + rng.uniform(0, 1) * du + rng.uniform(0, 1) * dv + rng.uniform(-0.1, 0.02) * n
        B = A + rng.normal(0, 0.05, 3)
        sl.append(np.stack([A, B, A + rng.uniform(0.2, 0.8) * (B - A) + 10.0 ** -rng.integers(4, 13) * rng.standard_normal(3)]))
    return np.concatenate([grid_wall(p0, du, dv), np.array(sl)])


SHAPES = ("generic", "sliver", "needle", "degenerate")
PLACES = ("unit", "cell", "offset1e3")
NAMES = {"far": [f"far_{s}_{p}" for p in PLACES for s in SHAPES],
         "lattice": ["lattice"],
         "contact": list(CONTACT_ORACLE_ERR),
         "traversal": ["traversal"]}


@functools.lru_cache(maxsize=None)
def family(name):
    """one family by name, generated once per process from a seed of its own (the far families call the exact reference to
    keep what is far)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.startswith("far_"):
        _, sname, place = name.split("_")
        return _far_family(name, _far_shapes(np.random.default_rng(11))[sname], place, rng, per_shape=12)
    if name == "lattice":
        return _lattice_family()
    if name == "contact_generic":
        return _contact_family(name, _generic(rng, 6), rng, ndir=5)
    if name.startswith("contact_sliver_"):
        return _contact_family(name, [_sliver(rng, float(name.rsplit("_", 1)[1])) for _ in range(6)], rng, ndir=5)
    assert name == "traversal", name
    return _traversal_family()


@functools.lru_cache(maxsize=None)
def exact(name):
    """exact distances of a (non-traversal) family, one array per case; computed once per process"""
    return [np.array([X.mesh_distance(s, tri) for s in segs]) for tri, segs in family(name).cases]
