"""GPU tests of moving mesh obstacles (cfs_problem_set_mesh_motion, include/cfs_hip.h): identity poses
against the static handle bit for bit, a constant pose against the mesh built from transformed vertices, varying poses and whole
solves against tests/mesh_motion_reference.py (whose cases tests/test_mesh_motion_reference.py vets on the CPU), and the handle's
state rules.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes as C

import numpy as np
import pytest

import mesh_motion_reference as M

pytestmark = pytest.mark.gpu

TOL_DIST, TOL_B, TOL_A = 1e-12, 1e-11, 5e-8     # tests/test_gpu_mesh.py's bars for dist / binq / Ainq
# grad = (d(+eps/2) - d(-eps/2)) / eps with eps = 1e-5: two distances within TOL_DIST each move it by at most 2e-12 / 1e-5
TOL_GRAD = 2e-7
ROBOT = "M200i"


class _Cell:
    """a handle with one line obstacle (main_FANUC's) and the given meshes, and the arrays of B copies of main_FANUC's problem"""

    def __init__(self, gpu, s, mode, tris, B=1, lines=(M.LINE,)):
        self.s, self.B, self.mode = s, B, mode
        self.meshes = [gpu.Mesh(tri=t) for t in tris]
        n = len(lines) + len(tris)
        self.h = gpu.CFSBatch(s, n, [M.EPS_MARGIN if mode == "CFS" else M.D_MARGIN] * n, mode=mode, max_batch=B)
        self.h.set_meshes(self.meshes)
        rows = [np.concatenate([l[:, 0], l[:, 1]]) for l in lines] + [np.zeros(6)] * len(tris)
        self.obs = np.tile(np.array(rows).reshape(1, n, 6), (B, 1, 1))
        rng = np.random.default_rng(5)
        self.x_init = np.tile(np.asarray(s.x_, float), (B, 1))
        self.x_init[1:] += 0.02 * rng.standard_normal((B - 1, self.x_init.shape[1]))     # problem 0 is main_FANUC's own
        self.xR1 = np.tile(s.xR1, (B, 1))
        self.ff, self.caug = np.tile(np.asarray(s.ff, float), (B, 1)), np.full(B, float(s.caug))
        self.noise = np.tile(M.noise_rows(s.H), (B, 1, 1)) if mode == "PSGCFS" else None

    def solve(self, idx=None):
        k = slice(None) if idx is None else slice(idx, idx + 1)
        return self.h.solve(self.x_init[k], self.xR1[k], self.ff[k], self.caug[k], self.obs[k],
                            noise=None if self.noise is None else self.noise[k])

    def everything(self):
        """every output of solve, linearize and get_con, as a flat list of arrays"""
        r = self.solve()
        lin = self.h.linearize(self.x_init, self.obs)
        con = self.h.get_con(self.x_init, np.zeros((self.B, self.h.nn)), self.xR1, self.obs)
        return [getattr(r, k) for k in ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")] + list(lin) + list(con)

    def close(self):
        self.h.close()
        for m in self.meshes:
            m.close()


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_identity_poses_are_the_static_handle_bit_for_bit(gpu, mode):
    import torch
    H, off, _, _ = M.CASES.cfs12
    c = _Cell(gpu, M.fanuc(gpu, H), mode, [M.post_and_ball(gpu.mesh, off), M.far_box(gpu.mesh)], B=3)
    static = c.everything()
    assert static[5].max() > 2                                      # iterations were taken: the comparison covers the loop
    c.h.set_mesh_motion([M.identity_poses(H), np.eye(4)])           # one (H, 4, 4) sequence, one 4x4 held over the horizon
    posed = c.everything()
    _same(static, posed)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    out = c.h.solve_device(t(c.x_init), t(c.xR1), t(c.ff), t(c.caug), t(c.obs), noise=None if c.noise is None else t(c.noise))
    torch.cuda.synchronize()
    _same(posed[:8], [getattr(out, k).cpu().numpy() for k in ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")])
    c.close()


def _constant_pose_case(gpu, s, mode, tri, T, lines, x_):
    a = _Cell(gpu, s, mode, [tri], lines=lines)
    a.h.set_mesh_motion([T])
    b = _Cell(gpu, s, mode, [M.transform(tri, T)], lines=lines)
    x_ = np.asarray(x_, float)[None]
    (da, la, ga), (db, lb, gb) = a.h.linearize(x_, a.obs), b.h.linearize(x_, b.obs)
    (Aa, ba), (Ab, bb) = a.h.get_con(x_, np.zeros((1, a.h.nn)), a.xR1, a.obs), b.h.get_con(x_, np.zeros((1, b.h.nn)), b.xR1, b.obs)
    print(f"dist {np.abs(da - db).max():.3g} binq {np.abs(ba - bb).max():.3g} Ainq {np.abs(Aa - Ab).max():.3g} grad {np.abs(ga - gb).max():.3g}")
    np.testing.assert_array_equal(la, lb)
    assert np.abs(da - db).max() < TOL_DIST and np.abs(ba - bb).max() < TOL_B and np.abs(Aa - Ab).max() < TOL_A
    assert np.abs(ga - gb).max() < TOL_GRAD
    a.close(), b.close()
    return da[0, -1]


def test_a_constant_pose_is_the_transformed_mesh_m200i(gpu):
    """the hierarchy differs (it is built from other vertices), the answer does not"""
    H, off, dy, ang = M.CASES.cfs12
    s = M.fanuc(gpu, H)
    T = M.poses_general(H, dy, ang)[H // 2]
    d = _constant_pose_case(gpu, s, "CFS", M.post_and_ball(gpu.mesh, off), T, (M.LINE,), s.x_)
    assert d.min() < M.EPS_MARGIN < d.max()                        # rows on both sides of the margin


def test_a_constant_pose_is_the_transformed_mesh_two_links(gpu):
    """another joint count (2L, njoint = 2), a box: main_2L's problem along the straight joint-space line"""
    R, s, obs = gpu.main_2L_problem()
    s.xR1 = np.concatenate([np.zeros(2), np.zeros(2)])
    x_ = gpu.line_reference(np.zeros(2), np.array([np.pi / 2, 0.0]), s.H)
    T = M.pose_about([1, 2, 3], [0.3, 0.3, 0.0], 0.5, [0.02, -0.03, 0.01])
    box = gpu.mesh.box_mesh([0.26, 0.27, -0.04], [0.34, 0.33, 0.05], n=2)
    d = _constant_pose_case(gpu, s, "CFS", box, T, (np.asarray(obs[0]["l"], float),), x_)
    assert d.min() < 0.25 and d.max() > 0.05


@pytest.fixture(scope="module")
def lin_handles(gpu):
    """the linearisation cases' handle: the post and ball (it moves) and a far box (held still), H = 30, and the same two meshes
    in the other order"""
    H, off, _, _ = M.CASES.lin
    s = M.fanuc(gpu, H)
    tri, box = M.post_and_ball(gpu.mesh, off), M.far_box(gpu.mesh)
    a, b = _Cell(gpu, s, "PSGCFS", [tri, box]), _Cell(gpu, s, "PSGCFS", [box, tri])
    yield s, tri, box, a, b
    a.close(), b.close()


@pytest.mark.parametrize("posefn", [M.poses_z, M.poses_general], ids=["vertical", "general-axis"])
def test_varying_poses_against_the_reference(gpu, O, lin_handles, posefn):
    s, tri, box, a, b = lin_handles
    H, _, dy, ang = M.CASES.lin
    P, I = posefn(H, dy, ang), M.identity_poses(H)
    a.h.set_mesh_motion([P, I])
    x_, u = np.asarray(s.x_, float), np.zeros(H * 5)
    dist, lid, grad = a.h.linearize(x_[None], a.obs)
    A, bq = a.h.get_con(x_[None], u[None], a.xR1, a.obs)
    so = M.fanuc(O, H)
    wA, wb, wd, wl, wg = M.get_con_posed(O, ROBOT, so, [M.LINE], [tri, box], [P, I], x_, u, "PSGCFS")
    print(f"dist {np.abs(dist[0] - wd).max():.3g} binq {np.abs(bq[0] - wb).max():.3g} Ainq {np.abs(A[0] - wA).max():.3g} "
          f"grad {np.abs(grad[0] - wg).max():.3g}")
    np.testing.assert_array_equal(lid[0, :1], wl[:1])               # linearize reports the closest link of line obstacles only
    assert np.abs(dist[0] - wd).max() < TOL_DIST and np.abs(bq[0] - wb).max() < TOL_B and np.abs(A[0] - wA).max() < TOL_A
    assert np.abs(grad[0] - wg).max() < TOL_GRAD
    assert wd[1].min() < M.D_MARGIN < wd[1].max() and wd[2].min() > 0.5          # the mover crosses its margin, the box is far
    # the two meshes in the other order: the rows are permuted and nothing else changes
    b.h.set_mesh_motion([I, P])
    d2, l2, g2 = b.h.linearize(x_[None], b.obs)
    A2, b2 = b.h.get_con(x_[None], u[None], b.xR1, b.obs)
    perm = [0, 2, 1]
    _same([dist, lid, grad], [d2[:, perm], l2[:, perm], g2[:, perm]])
    per = H * (1 + 2 * 5)
    _same([A.reshape(3, per, -1), bq.reshape(3, per)], [A2.reshape(3, per, -1)[perm], b2.reshape(3, per)[perm]])


@pytest.fixture(scope="module")
def psg_case(gpu, O):
    """the vetted PSGCFS case: the device's posed and snapshot plans and the reference's posed plan (one reference solve per module)"""
    H, off, dy, ang = M.CASES.psg
    tri, P = M.post_and_ball(gpu.mesh, off), M.poses_z(H, dy, ang)
    c = _Cell(gpu, M.fanuc(gpu, H), "PSGCFS", [tri])
    snap = c.solve()
    c.h.set_mesh_motion([P])
    posed = c.solve()
    so = M.fanuc(O, H)
    want = M.optimizer_posed(O, ROBOT, so, [M.LINE], [tri], [P], "PSGCFS", so.x_, noise=M.noise_rows(H))
    yield so, tri, P, snap, posed, want
    c.close()


def test_cfs_whole_solve_against_the_reference(gpu, O):
    H, off, dy, ang = M.CASES.cfs12
    tri, P = M.post_and_ball(gpu.mesh, off), M.poses_z(H, dy, ang)
    c = _Cell(gpu, M.fanuc(gpu, H), "CFS", [tri])
    c.h.set_mesh_motion([P])
    got = c.solve()
    so = M.fanuc(O, H)
    want = M.optimizer_posed(O, ROBOT, so, [M.LINE], [tri], [P], "CFS", so.x_)
    print(f"status {want.status} iter_O {want.iter_O} x_ {np.abs(got.x_[0] - want.x_).max():.3g}")
    assert got.status[0] == want.status == 0 and got.iter_O[0] == want.iter_O and want.iter_O > 3
    assert np.abs(got.x_[0] - want.x_).max() < 1e-7
    np.testing.assert_allclose(got.cost_all[0, :want.iter_O - 1], want.cost_all, rtol=1e-9)
    c.close()


def test_psgcfs_whole_solve_against_the_reference(psg_case):
    so, tri, P, snap, posed, want = psg_case
    print(f"status {want.status} iter_O {want.iter_O} x_ {np.abs(posed.x_[0] - want.x_).max():.3g}")
    assert posed.status[0] == want.status == 1 and posed.iter_O[0] == want.iter_O == 21
    assert np.abs(posed.x_[0] - want.x_).max() < 1e-5


def test_the_posed_plan_keeps_the_margin_where_the_snapshot_plan_cuts_it(O, psg_case):
    so, tri, P, snap, posed, want = psg_case
    d_snap = M.clearance_where_it_is(O, so, [tri], [P], snap.x_[0])
    d_posed = M.clearance_where_it_is(O, so, [tri], [P], posed.x_[0])
    print(f"snapshot {d_snap:.4f} posed {d_posed:.4f}")
    assert d_snap < M.D_MARGIN - 0.02                               # planned against the mesh as stored
    assert d_posed > M.D_MARGIN - 1e-3                              # tests/test_gpu_moving.py's linearisation bound


@pytest.fixture(scope="module")
def cfs3(gpu):
    """B = 3 problems with different x_init against the moving post and a still box, H = 12"""
    H, off, dy, ang = M.CASES.cfs12
    c = _Cell(gpu, M.fanuc(gpu, H), "CFS", [M.post_and_ball(gpu.mesh, off), M.far_box(gpu.mesh)], B=3)
    c.poses = [M.poses_z(H, dy, ang), M.identity_poses(H)]
    c.h.set_mesh_motion(c.poses)
    yield c
    c.close()


def _fields(r):
    return [getattr(r, k) for k in ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")]


def test_every_problem_of_a_batch_equals_its_own_solve_and_the_same_call_twice_the_same_bits(cfs3):
    whole = _fields(cfs3.solve())
    assert len({tuple(x) for x in whole[1]}) == 3                   # three different plans
    _same(whole, _fields(cfs3.solve()))                             # determinism
    for b in range(3):
        _same([f[b:b + 1] for f in whole], _fields(cfs3.solve(b)))


def test_return_to_static(gpu, cfs3):
    posed = cfs3.everything()
    cfs3.h.set_mesh_motion(None)
    static = cfs3.everything()
    assert np.abs(static[1] - posed[1]).max() > 1e-3                # the motion mattered
    cfs3.h.set_mesh_motion(cfs3.poses)
    _same(posed, cfs3.everything())
    cfs3.h.set_meshes(cfs3.meshes)                                  # every set_meshes resets the handle to static
    _same(static, cfs3.everything())
    cfs3.h.clearance_mesh(static[1], static[0], cfs3.xR1, cfs3.obs, substeps=2)     # and the audit takes it again
    cfs3.h.set_mesh_motion(cfs3.poses)


def test_refusals_on_a_live_handle_change_nothing(gpu, cfs3):
    h, lib, H = cfs3.h, gpu.lib(), cfs3.s.H
    before = cfs3.everything()
    good = np.stack([gpu.mesh_pose_array(p, H) for p in cfs3.poses])

    def refused(arr, word):
        arr = np.ascontiguousarray(arr, np.float64)
        assert lib.cfs_problem_set_mesh_motion(h._h, arr.ctypes.data_as(C.c_void_p)) == -1
        assert word in lib.cfs_last_error()

    for at, value in [((1, 3, 7), np.nan), ((0, 0, 0), np.inf)]:
        bad = good.copy()
        bad[at] = value
        refused(bad, b"not finite")
    scaled = good.copy().reshape(2, H, 3, 4)
    scaled[0, 5, :, :3] *= 1.0 + 1e-8                               # max|RR' - I| = 2e-8 > 1e-9
    refused(scaled, b"rigid")
    mirrored = good.copy().reshape(2, H, 3, 4)
    mirrored[1, H - 1, :, 0] *= -1.0                                # orthogonal, det R = -1
    refused(mirrored, b"rigid")
    assert lib.cfs_problem_set_mesh_motion(None, good.ctypes.data_as(C.c_void_p)) == -1
    with pytest.raises(ValueError):
        h.set_mesh_motion([good[0]])                                # one sequence for two meshes
    with pytest.raises(ValueError):
        h.clearance_mesh(before[1], before[0], cfs3.xR1, cfs3.obs)
    z = np.zeros((3, h.nobs))
    zi = np.zeros((3, h.nobs), np.int32)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cfs_clearance_mesh(h._h, 3, 4, p(before[1]), p(before[0]), p(cfs3.xR1), p(cfs3.obs), p(z), p(z), p(z), p(z), p(zi), p(zi)) == -1
    assert b"mesh motion" in lib.cfs_last_error() and not z.any()
    with pytest.raises(gpu.CfsError):
        h.set_obstacle_motion("per_waypoint")                       # lines stay static in a handle whose meshes move
    with pytest.raises(gpu.CfsError):
        h.set_infeasible_policy("soften", 1e4)
    _same(before, cfs3.everything())
    bare = gpu.CFSBatch(cfs3.s, 1, [M.EPS_MARGIN], mode="CFS")      # a handle without meshes
    assert lib.cfs_problem_set_mesh_motion(bare._h, good.ctypes.data_as(C.c_void_p)) == -1
    assert b"mesh obstacles" in lib.cfs_last_error()
    with pytest.raises(ValueError):
        bare.set_mesh_motion([np.eye(4)])
    bare.close()
