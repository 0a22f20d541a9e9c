"""GPU: the mesh distance queries of cfs_mesh_dev.h on hard geometry (mesh_geometry_cases.py): against the exact rational
reference (mesh_exact_reference.py) where one triangle is measured, against the brute-force oracle where the hierarchy is
what is tested -- flat walls whose boxes have zero thickness, ties among many triangles, slivers, leaf boundaries, queries on
slab boundaries -- and through the features that share those device functions (dist_arm_surf, the linearisation with an
overflowing near-tie list, a whole CFS solve).

The library holds two builds of the query kernel, and every check of distances runs on both:
  contracted   cfs_debug_mesh_segment_distance_contracted: FMA contraction on, the arithmetic in which dist_arm_surf, the
               linearisation, the clearance audits, IK and the Cartesian moves run seg_tri_update, closest_pt_triangle,
               seg_seg_full, node_lower_bound and mesh_query.  Whether node_lower_bound stays below the distances that
               seg_tri_update computes depends on how the build rounds, so this is the build the pruning checks are about.
  public       cfs_mesh_segment_distance: no contraction, it rounds like the oracle.  Only this build is held to the oracle's
               first point and to the oracle's distances bit for bit.

Run on the GPU box:  python -m pytest tests/test_gpu_mesh_geometry.py -m gpu -q -s
"""
import ctypes as C

import numpy as np
import pytest

import mesh_geometry_cases as G

pytestmark = pytest.mark.gpu

TOL_DIST = 1e-12      # metres, device against oracle: the suite's bound for the same formulas in fp64 (test_gpu_mesh.py)
OID, OID1 = 11, 12    # oracle mesh slots of this module (0 .. 10 and 13 belong to the other test modules)
BUILDS = ["contracted", "public"]


def _device(gpu, tri, segs, build):
    """(dis, points, tri) of the segments against the mesh, from one of the two builds of the query kernel"""
    m = gpu.Mesh(tri=tri)
    if build == "public":
        out = m.point2surface_dis(segs)
    else:
        segs = np.ascontiguousarray(segs, np.float64)
        n = segs.shape[0]
        out = np.zeros(n), np.zeros((n, 6)), np.zeros(n, np.int32)
        p = [a.ctypes.data_as(C.c_void_p) for a in (segs,) + out]
        gpu._lib.check(m._lib.cfs_debug_mesh_segment_distance_contracted(m._h, n, *p))
    m.close()
    return out


def _device_errors(gpu, name, build):
    """per case of a family: (tri, segs, |device - exact|)"""
    return [(tri, segs, np.abs(_device(gpu, tri, segs, build)[0] - ex)) for (tri, segs), ex in zip(G.family(name).cases, G.exact(name))]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", G.NAMES["far"] + G.NAMES["lattice"])
def test_segment_distance_against_exact_away_from_contact(gpu, name, build):
    """16 eps L, L the largest |coordinate| of the pair: the forward error of well-conditioned fp64 formulas of this depth"""
    worst = 0.0
    for tri, segs, err in _device_errors(gpu, name, build):
        L = np.array([G.coord_scale(tri, s) for s in segs])
        worst = max(worst, float((err / L).max()))
        assert np.all(err <= 16 * G.EPS * L), (name, float((err / (G.EPS * L)).max()))
    print(f"{name} {build}: worst device error {worst / G.EPS:.2f} eps L")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", G.NAMES["contact"])
def test_segment_distance_against_exact_near_contact(gpu, name, build):
    """4x the oracle's own worst error on the family (measured on the CPU, mesh_geometry_cases.CONTACT_ORACLE_ERR), floor
    TOL_DIST: contracted multiply-adds re-round the same ill-conditioned predicates, so the device may decide them otherwise"""
    tol = max(4 * G.CONTACT_ORACLE_ERR[name], TOL_DIST)
    worst = max(float(err.max()) for _, _, err in _device_errors(gpu, name, build))
    print(f"{name} {build}: worst device error {worst:.3e} m (bound {tol:.1e})")
    assert worst <= tol


def _single_triangle_distance(O, tri, tid, segs):
    """the oracle's distance of every segment to the one triangle tri[tid[i]]"""
    out = np.zeros(len(tid))
    for t in np.unique(tid):
        sel = tid == t
        O.mesh_register(OID1, tri[t][None])
        out[sel] = O.mesh_seg_distance(OID1, segs[sel])[0]
    return out


PARTS = {"walls": slice(0, 4), "soups": slice(4, 19), "counts": slice(19, None)}


@pytest.fixture(scope="module")
def traversal(gpu, O):
    """every case of the traversal family measured once: build -> [(tri, segs, oracle (dis, pts, tri), device (dis, pts, tri))]"""
    out = {b: [] for b in BUILDS}
    for tri, segs in G.family("traversal").cases:
        O.mesh_register(OID, tri)
        want = O.mesh_seg_distance(OID, segs)
        for b in BUILDS:
            out[b].append((tri, segs, want, _device(gpu, tri, segs, b)))
    return out


def _point_segment(p, segs):
    a, d = segs[:, :3], segs[:, 3:] - segs[:, :3]
    D = np.einsum("ij,ij->i", d, d)
    t = np.clip(np.einsum("ij,ij->i", p - a, d) / np.where(D > 0, D, 1.0), 0.0, 1.0)
    return np.linalg.norm(a + t[:, None] * d - p, axis=1)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("part", list(PARTS))
def test_traversal_against_brute_force(O, traversal, part, build):
    """the hierarchy only prunes: distance, closest pair and triangle are what the brute force over every triangle finds"""
    worst_d = worst_p = worst_t = 0.0
    for tri, segs, (od, _, _), (dis, pts, tid) in traversal[build][PARTS[part]]:
        assert dis.shape == (segs.shape[0],)
        worst_d = max(worst_d, float(np.abs(dis - od).max()))
        assert np.abs(dis - od).max() < TOL_DIST, (tri.shape[0], segs.shape[0])     # a larger device distance is a pruned triangle
        far = od > 1e-6
        if far.any():
            np.testing.assert_allclose(np.linalg.norm(pts[far, :3] - pts[far, 3:], axis=1), dis[far], rtol=0, atol=1e-12)
        # the reported pair is a closest pair whatever the ties: a point of the axis at the minimum distance, a point of the mesh
        assert _point_segment(pts[:, :3], segs).max() < TOL_DIST * max(1.0, np.abs(segs).max())
        O.mesh_register(OID, tri)
        d_axis = O.mesh_seg_distance(OID, np.concatenate([pts[:, :3], pts[:, :3]], axis=1))[0]
        d_mesh = O.mesh_seg_distance(OID, np.concatenate([pts[:, 3:], pts[:, 3:]], axis=1))[0]
        worst_p = max(worst_p, float(np.abs(d_axis - dis).max()), float(d_mesh.max()))
        assert np.abs(d_axis - dis).max() < TOL_DIST * max(1.0, np.abs(segs).max()) and d_mesh.max() < TOL_DIST
        assert tid.min() >= 0 and tid.max() < tri.shape[0]
        dt = _single_triangle_distance(O, tri, tid, segs)                          # the reported triangle attains the minimum
        worst_t = max(worst_t, float(np.abs(dt - dis).max()))
        assert np.abs(dt - dis).max() < TOL_DIST
    print(f"traversal {part} {build}: worst |dis - oracle| {worst_d:.2e}, closest pair off by {worst_p:.2e}, |dis(tri) - dis| {worst_t:.2e}")


@pytest.mark.parametrize("part", list(PARTS))
def test_traversal_first_point_against_brute_force(traversal, part):
    """The contract's "smaller parameter along the axis": pts[:3] of the public query equals the oracle's within 1e-9, and its
    distances equal the oracle's in every bit.

    Only the public build is asked.  Where a segment lies in the surface, or parallel to a wall or to an edge, a continuum of
    axis points is at the minimum distance; in fp64 their distances differ in the last bits, and which is smallest is decided
    by rounding.  Two implementations name the same point there only if they round alike: the public query is built without
    FMA contraction, as the oracle is, for this reason (csrc/cfs_mesh_query.hip).  The contracted build reports another of the
    tied points on about 1 % of these queries, up to a whole segment away, at the same distance to 2e-15; that its point is a
    closest point all the same is what test_traversal_against_brute_force asserts of both builds."""
    worst, n_off = 0.0, 0
    for tri, segs, (_, op, _), (_, pts, _) in traversal["public"][PARTS[part]]:
        e = np.abs(pts[:, :3] - op[:, :3]).max(axis=1)
        worst, n_off = max(worst, float(e.max())), n_off + int((e > 1e-9).sum())
    print(f"traversal {part}: worst |pts[:3] - oracle| {worst:.2e} m, {n_off} queries off by more than 1e-9")
    for tri, segs, (od, op, _), (dis, pts, _) in traversal["public"][PARTS[part]]:
        np.testing.assert_allclose(pts[:, :3], op[:, :3], rtol=0, atol=1e-9)
        np.testing.assert_array_equal(dis, od)


# ---- through the features that share the device functions ---------------------------------------------------------------
def _link_distances(O, orobot, th, mesh_id):
    """raw (before the near-zero surrogate) distance of every link axis of every pose to the registered mesh: (N, nlink)"""
    pos = np.stack([O.arm_pos(orobot, t) for t in th])                              # (N, nlink, 2, 3)
    d = O.mesh_seg_distance(mesh_id, pos.reshape(-1, 6))[0]
    return d.reshape(th.shape[0], -1)


@pytest.mark.parametrize("which", ["flat", "sliver"])
def test_dist_arm_surf_on_walls(gpu, O, which):
    robot, orobot = gpu.robotproperty2("M200i"), O.robotproperty2("M200i")
    tri = G.flat_wall() if which == "flat" else G.sliver_wall()
    l = O.mesh_register(14, tri)
    rng = np.random.default_rng(21)
    th = np.array([0.0, 0.0, 0.2, 0.1, -1.1]) + rng.uniform(-0.9, 0.9, (200, 5))
    # a link whose distance sits on the 1e-4 threshold of the surrogate may fall on either side of it: such poses are dropped
    keep = np.all(np.abs(_link_distances(O, orobot, th, 14) - 1e-4) > 1e-9, axis=1)
    assert keep.sum() >= 190                                                        # at most 5 % (this seed: none)
    th = th[keep]
    m = gpu.Mesh(tri=tri)
    d, lid, _ = gpu.dist_arm_surf(robot, th, m)
    m.close()
    neg = 0
    for n in range(th.shape[0]):
        dd, ll = O.dist_arm(orobot, th[n], l)
        assert abs(d[n] - dd) < 1e-11 and lid[n] == ll, (n, d[n], dd, lid[n], ll)
        neg += dd < 0
    assert neg >= 3                                                                 # poses that reach the wall: the surrogate branch


def _forearm_wall(O, P, sliver):
    """a 32 x 32 wall parallel to the forearm of main_FANUC's first waypoint, 0.25 m above it: 0.75 m along the axis, of which
    0.3 m are over the forearm (the wrist end is left uncovered: the wrist's upper end stands 9 mm above the forearm's axis
    and would be the closer link), 0.4 m across.  The 51 triangles under the covered part of the axis tie."""
    th0 = np.asarray(P.sys_info.x_).reshape(P.sys_info.H, -1)[0, :5]
    pos = O.arm_pos(P.sys_info.robot, th0)
    a, b = pos[3, 1], pos[3, 0]                                                     # the forearm, elbow to wrist: 0.4 m
    d = (b - a) / np.linalg.norm(b - a)
    e = np.array([-d[1], d[0], 0.0]) / np.hypot(d[0], d[1])                         # horizontal, across the axis
    n = np.cross(d, e)                                                              # up, square to the axis
    assert n[2] > 0.9
    p0 = a + 0.25 * n - 0.45 * d - 0.2 * e
    tri = (G.sliver_wall if sliver else G.flat_wall)(p0, 0.75 * d, 0.4 * e)         # d x e = n: the slivers hang on the arm's side
    return tri, np.concatenate([a, b])


def _wall_problem(gpu, O, sliver):
    R, s, obs = gpu.main_FANUC_problem()
    P = O.problem_main_FANUC()
    tri, forearm = _forearm_wall(O, P, sliver)
    l = O.mesh_register(15, tri)
    # margins below the 0.25 m of the wall: the first waypoint is fixed, and a margin equal to its distance would put the
    # feasibility of the linearisation on a rounding error
    g_obs = obs + [dict(mesh=gpu.Mesh(tri=tri), D=0.15, epsilon=0.2)]
    o_obs = [dict(l=o["l"], D=o["D"], epsilon=o["epsilon"]) for o in obs] + [dict(l=l, D=0.15, epsilon=0.2)]
    return R, s, g_obs, P, o_obs, tri, forearm


@pytest.mark.parametrize("sliver", [False, True])
def test_get_con_with_a_wall_along_the_forearm(gpu, O, sliver):
    R, s, g_obs, P, o_obs, tri, forearm = _wall_problem(gpu, O, sliver)
    if not sliver:
        # The linearisation queries a link axis in 4 equal pieces (CFS_MESH_PIECES), each with a near-tie list of its own of
        # NEAR_CAP = 12 entries: the overflow path runs only if MORE THAN 12 TRIANGLES TIE FOR ONE PIECE.  Counted here with the
        # oracle, so that another wall size or piece count cannot silently stop exercising it.
        O.mesh_register(OID1, tri)
        assert abs(O.mesh_seg_distance(OID1, forearm[None])[0][0] - 0.25) < 1e-12
        a, d = forearm[:3], forearm[3:] - forearm[:3]
        pieces = np.array([np.concatenate([a + k / 4 * d, a + (k + 1) / 4 * d]) for k in range(4)])
        pmin = O.mesh_seg_distance(OID1, pieces)[0]
        ties = np.zeros(4, int)
        for T in tri:
            O.mesh_register(OID1, T[None])
            ties += O.mesh_seg_distance(OID1, pieces)[0] <= pmin + 1e-9
        assert ties.max() > 12, ties
    slv = gpu.CFS_FANUC(g_obs, s, R)
    slv.get_con()
    A, b, dist, lid, grad = O.get_con(P.ROBOT, P.sys_info, o_obs, P.sys_info.x_, np.zeros(s.H * s.nu))
    assert slv.Ainq.shape == A.shape
    np.testing.assert_allclose(slv.binq, b, rtol=0, atol=1e-11)
    np.testing.assert_allclose(slv.Ainq, A, rtol=0, atol=5e-8)                      # finite differences: eps = 1e-5 amplifies 1e-13
    d_g, _, g_g = slv._batch.linearize(np.asarray(s.x_)[None], gpu.obs_to_array(g_obs)[None])
    np.testing.assert_allclose(d_g[0], dist, rtol=0, atol=1e-12)
    assert np.abs(d_g[0][-1]).max() > 0.05                                          # the mesh rows are real distances
    if not sliver:
        assert abs(d_g[0][-1][0] - 0.25) < 1e-9                                     # the first waypoint is the tie
    del slv
    g_obs[-1]["mesh"].close()


def test_cfs_against_a_wall_along_the_forearm(gpu, O):
    R, s, g_obs, P, o_obs, _, _ = _wall_problem(gpu, O, False)
    got = gpu.CFS_FANUC(g_obs, s, R).optimizer()
    want = O.optimizer(P.ROBOT, P.sys_info, o_obs, "CFS")
    assert got.status == want.status and got.iter_O == want.iter_O
    assert np.abs(got.x_ - want.x_).max() < 1e-6
    g_obs[-1]["mesh"].close()
