"""Moving meshes at the Python surface and at the C entry, without a device: the pose arrays, every refusal that happens before the
library is asked, the solvers that have no time axis, and the state the bindings keep (CPU)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_motion_reference as M
import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib, solvers
from test_ik_args import LINE, ROBOT
from test_ik_mesh_args import _mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 7
POSES = M.poses_general(H, -0.3, 0.6)


def test_entry_point_is_exported_bound_and_described():
    assert hasattr(C.CDLL(_lib.LIB_PATH), "cfs_problem_set_mesh_motion")
    assert "cfs_problem_set_mesh_motion" in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive
    src = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_problem_set_mesh_motion(cfs_problem *p, const double *poses);" in src
    assert "bit for bit the static handle's" in src and "x_world = R x_mesh + t" in src
    assert pkg.mesh_pose_array is solvers.mesh_pose_array and "mesh_pose_array" in pkg.__all__


def test_null_handle_is_refused_by_the_library():
    lib = pkg.lib()
    poses = np.ascontiguousarray(POSES[:, :3, :])
    assert lib.cfs_problem_set_mesh_motion(None, poses.ctypes.data_as(C.c_void_p)) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert lib.cfs_problem_set_mesh_motion(None, None) == -1


def test_mesh_pose_array_shapes_layout_and_broadcast():
    a = pkg.mesh_pose_array(POSES, H)
    assert a.shape == (H, 12) and a.dtype == np.float64 and a.flags.c_contiguous
    np.testing.assert_array_equal(a.reshape(H, 3, 4), POSES[:, :3, :])   # row-major [R | t]
    np.testing.assert_array_equal(pkg.mesh_pose_array(POSES[:, :3, :], H), a)
    one = pkg.mesh_pose_array(POSES[3], H)                                # a single 4x4 is held over the horizon
    assert one.shape == (H, 12) and (one == a[3]).all()
    np.testing.assert_array_equal(pkg.mesh_pose_array(POSES[3][:3], H), one)
    np.testing.assert_array_equal(pkg.mesh_pose_array(np.eye(4), H), np.tile(np.eye(4)[:3].reshape(-1), (H, 1)))
    np.testing.assert_array_equal(pkg.mesh_pose_array(POSES.tolist(), H), a)


def _bad(change):
    P = POSES.copy()
    change(P)
    return P


@pytest.mark.parametrize("pose", [
    POSES[:-1], POSES[:, :, :3], POSES[:, :2], np.zeros((H, 12)), np.eye(3), "pose", None, [[1, 2], [3]],
    _bad(lambda P: P.__setitem__((2, 1, 3), np.nan)), _bad(lambda P: P.__setitem__((0, 0, 0), np.inf)),
    _bad(lambda P: P.__setitem__((4, 3, 3), 2.0)), _bad(lambda P: P.__setitem__((4, 3, 0), 1e-3)),          # last row not [0 0 0 1]
    _bad(lambda P: P[1, :3, :3].__imul__(1.0 + 1e-8)),                                                     # scaled
    _bad(lambda P: P[1, :3, :3].__imul__(2.0)),
    _bad(lambda P: P[5, :3, 0].__imul__(-1.0)),                                                            # mirrored: det R = -1
    _bad(lambda P: P.__setitem__((6, 0, 1), P[6, 0, 1] + 1e-6)),                                            # sheared
    np.diag([1.0, 1.0, 0.0, 1.0]),                                                                          # flattened: det R = 0
], ids=lambda p: None)
def test_mesh_pose_array_refuses(pose):
    with pytest.raises(ValueError):
        pkg.mesh_pose_array(pose, H)


def test_a_rotation_within_rounding_is_accepted():
    P = POSES.copy()
    P[:, :3, :3] *= 1.0 + 1e-12                                           # max|RR' - I| = 2e-12 <= 1e-9
    pkg.mesh_pose_array(P, H)


class _FakeLib:
    """records the calls that reach the library and answers success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a))
            return 0
        return call


class _Handle(pkg.CFSBatch):
    obstacle_motion = "static"

    def __init__(self, nmesh):
        self.H, self.nj, self.ns, self.nn, self.nx, self.nobs, self.max_batch = H, 5, 10, 5 * H, 10 * H, 3, 2
        self.margin = np.full(3, 0.2)
        self._lib, self._h = _FakeLib(), None
        if nmesh is not None:
            self.set_meshes([_mesh() for _ in range(nmesh)])

    def close(self):
        pass

    __del__ = close


def test_set_mesh_motion_packs_nmesh_by_H_by_12_and_none_clears():
    h = _Handle(2)
    h.set_mesh_motion([POSES, np.eye(4)])
    name, (hd, ptr) = h._lib.calls[-1]
    assert name == "cfs_problem_set_mesh_motion" and h._mesh_motion
    got = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(2, H, 12)).copy()
    np.testing.assert_array_equal(got[0], pkg.mesh_pose_array(POSES, H))
    np.testing.assert_array_equal(got[1], pkg.mesh_pose_array(np.eye(4), H))
    h.set_mesh_motion(np.stack([pkg.mesh_pose_array(POSES, H)] * 2))       # (nmesh, H, 12) as the library takes it
    assert h._lib.calls[-1][0] == "cfs_problem_set_mesh_motion"
    h.set_mesh_motion(None)
    assert h._lib.calls[-1] == ("cfs_problem_set_mesh_motion", (None, None)) and not h._mesh_motion


def test_set_mesh_motion_refuses_before_the_library():
    for h in (_Handle(None), _Handle(0)):                                 # set_meshes never called / called with none
        n = len(h._lib.calls)
        with pytest.raises(ValueError, match="mesh"):
            h.set_mesh_motion([np.eye(4)])
        with pytest.raises(ValueError, match="mesh"):
            h.set_mesh_motion(None)
        assert len(h._lib.calls) == n
    h = _Handle(2)
    n = len(h._lib.calls)
    for bad in ([POSES], [POSES, POSES, POSES], [POSES, POSES[:-1]], [POSES, 2.0 * np.eye(4)]):
        with pytest.raises(ValueError):
            h.set_mesh_motion(bad)
    assert len(h._lib.calls) == n and not h._mesh_motion


def test_set_meshes_resets_the_motion_and_the_audit_refuses_a_moving_handle():
    h = _Handle(1)
    h.set_mesh_motion([POSES])
    arrays = np.zeros((2, 10 * H)), np.zeros((2, 5 * H)), np.zeros((2, 10)), np.zeros((2, 3, 6))
    n = len(h._lib.calls)
    with pytest.raises(ValueError, match="mesh motion"):
        h.clearance_mesh(*arrays)
    assert len(h._lib.calls) == n
    h.set_meshes(h._meshes)
    assert not h._mesh_motion
    h.clearance_mesh(*arrays)                                             # static again: the call reaches the library
    assert h._lib.calls[-1][0] == "cfs_clearance_mesh"


@pytest.mark.parametrize("cls", ["CFS_FANUC", "PSGCFS_FANUC"])
def test_solver_classes_take_pose_entries_and_hold_the_others_still(cls, monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    P = M.poses_z(s.H, -0.3, 0.6)
    calls = []
    stub = SimpleNamespace(set_meshes=lambda m: calls.append(("meshes", len(m))), set_mesh_motion=lambda p: calls.append(("motion", p)))
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: stub)
    cell = obs + [dict(mesh=_mesh(), epsilon=0.25, D=0.2), dict(mesh=_mesh(), epsilon=0.25, D=0.2, pose=P)]
    getattr(pkg, cls)(cell, s, R)
    assert [c[0] for c in calls] == ["meshes", "motion"] and calls[0][1] == 2
    sent = calls[1][1]
    assert sent.shape == (2, s.H, 12)
    np.testing.assert_array_equal(sent[0], pkg.mesh_pose_array(np.eye(4), s.H))      # no pose: the identity
    np.testing.assert_array_equal(sent[1], pkg.mesh_pose_array(P, s.H))
    calls.clear()
    getattr(pkg, cls)(cell[:2], s, R)                                     # no entry with a pose: the handle is never told
    assert [c[0] for c in calls] == ["meshes"]


@pytest.mark.parametrize("cls", ["CFS_FANUC", "PSGCFS_FANUC"])
def test_solver_classes_refuse_before_the_device(cls, monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    P = M.poses_z(s.H, -0.3, 0.6)
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="audit_mesh"):                   # the audit's bound assumes meshes that stand still
        getattr(pkg, cls)(obs + [dict(mesh=_mesh(), epsilon=0.25, D=0.2, pose=P)], s, R, audit_mesh=8)
    for bad in (P[:-1], 1.001 * P, np.diag([1.0, -1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            getattr(pkg, cls)(obs + [dict(mesh=_mesh(), epsilon=0.25, D=0.2, pose=bad)], s, R)
    moving_line = dict(obs[0], l=np.repeat(np.asarray(obs[0]["l"], float)[:, :, None], s.H, axis=2))
    with pytest.raises(ValueError):                                       # moving lines and moving meshes do not mix
        getattr(pkg, cls)([moving_line, dict(mesh=_mesh(), epsilon=0.25, D=0.2, pose=P)], s, R)
    assert not touched


def test_solvers_without_a_time_axis_refuse_a_mesh_with_a_pose():
    pobs, s, g, region_g, region_s, off = pkg.RRTstar_problem()
    mesh_still = dict(mesh=_mesh(), D=0.1, epsilon=0.1)
    mesh_moving = dict(mesh_still, pose=np.eye(4))                        # even the identity: a pose is a claim about time
    for make in (lambda c: pkg.RRT_FANUC(c, s, g, region_g, region_s, off, "M200i", "RRT"),
                 lambda c: pkg.s_Parallel_rrt(c, s, g, region_g, region_s, off, "M200i"),
                 lambda c: pkg.RRTCFSPlanner(c, s, region_g, region_s, off),
                 lambda c: pkg.IKSolver(ROBOT, [LINE] + c[-1:]),
                 lambda c: pkg.CartesianPath(ROBOT, [LINE] + c[-1:], meshes=True)):
        with pytest.raises(ValueError, match="pose"):
            make(list(pobs) + [mesh_moving])
    pkg.RRT_FANUC(list(pobs) + [mesh_still], s, g, region_g, region_s, off, "M200i", "RRT")     # the same cell without the pose
    pkg.IKSolver(ROBOT, [LINE, mesh_still])
