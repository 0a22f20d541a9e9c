"""The clearance audit with moving meshes at the Python surface and at the C entry, without a device: the entry points exist and are
bound, the new surfaces (CFSBatch.clearance_mesh_motion / clearance_mesh_motion_device, audit_mesh_motion= of the solver classes)
reach cfs_clearance_mesh_motion, every refusal happens before the library is asked, and the static audit keeps refusing a moving
handle (CPU)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_motion_reference as M
import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib, solvers
from test_ik_mesh_args import _mesh
from test_mesh_motion_args import H, POSES, _Handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(B=2):
    return np.zeros((B, 10 * H)), np.zeros((B, 5 * H)), np.zeros((B, 10)), np.zeros((B, 3, 6))


def test_entry_points_are_exported_bound_and_described():
    h = C.CDLL(_lib.LIB_PATH)
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("cfs_clearance_mesh_motion", "cfs_clearance_mesh_motion_device"):
        assert hasattr(h, n) and n in names
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive
    src = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "clearance audit with moving meshes" in src and "int cfs_clearance_mesh_motion_device(" in src
    assert "v_mesh" in src and "quarter turn" in src


def test_null_handle_is_refused_and_nothing_is_written():
    lib = pkg.lib()
    z = np.zeros(64)
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.cfs_clearance_mesh_motion(None, 1, 16, p, p, p, p, p, p, p, p, p, p) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert lib.cfs_clearance_mesh_motion_device(None, 1, 16, p, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert (z == 0).all()


def test_a_moving_and_a_static_handle_reach_the_new_entry_with_every_array():
    for moving in (True, False):
        h = _Handle(1)
        if moving:
            h.set_mesh_motion([POSES])
        x_, u, xR1, obs = _arrays()
        out = h.clearance_mesh_motion(x_, u, xR1, obs, substeps=5)
        name, a = h._lib.calls[-1]
        assert name == "cfs_clearance_mesh_motion" and a[1:3] == (2, 5) and len(a) == 13
        assert [q.value for q in a[3:7]] == [t.ctypes.data for t in (x_, u, xR1, obs)]
        names = ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path", "tri_path")
        assert [q.value for q in a[7:]] == [getattr(out, k).ctypes.data for k in names]
        assert all(getattr(out, k).shape == (2, 3) for k in names) and out.tri_path.dtype == np.int32
        np.testing.assert_array_equal(out.short_by, np.full(2, 0.2))     # margin - dist_path of the zeros the fake left
        assert h.clearance_mesh_motion(x_, u, xR1, obs).dist_wp.shape == (2, 3) and h._lib.calls[-1][1][2] == 16   # the default


def test_the_static_audit_keeps_refusing_a_moving_handle():
    h = _Handle(1)
    h.set_mesh_motion([POSES])
    n = len(h._lib.calls)
    with pytest.raises(ValueError, match="mesh motion"):
        h.clearance_mesh(*_arrays())
    with pytest.raises(ValueError, match="mesh motion"):
        h.clearance_mesh_device(*_arrays())
    assert len(h._lib.calls) == n


@pytest.mark.parametrize("S", [0, -1, 65, 1000, 16.0, "16", None, True, np.nan])
def test_bad_substeps_are_refused_before_the_library(S):
    h = _Handle(1)
    h.set_mesh_motion([POSES])
    n = len(h._lib.calls)
    with pytest.raises(ValueError, match="substeps"):
        h.clearance_mesh_motion(*_arrays(), substeps=S)
    with pytest.raises(ValueError, match="substeps"):
        h.clearance_mesh_motion_device(*_arrays(), substeps=S)           # refused before the tensors are looked at
    assert len(h._lib.calls) == n


def test_handles_without_meshes_and_bad_shapes_are_refused_before_the_library():
    for h in (_Handle(None), _Handle(0)):
        n = len(h._lib.calls)
        with pytest.raises(ValueError, match="clearance_mesh_motion needs a handle with mesh"):
            h.clearance_mesh_motion(*_arrays())
        with pytest.raises(ValueError, match="mesh"):
            h.clearance_mesh_motion_device(*_arrays())
        assert len(h._lib.calls) == n
    h = _Handle(1)
    h.set_mesh_motion([POSES])
    n = len(h._lib.calls)
    x_, u, xR1, obs = _arrays()
    for bad in ((x_[:, :-1], u, xR1, obs), (x_, u[:1], xR1, obs), (x_, u, xR1[:, :5], obs), (x_, u, xR1, obs[:, :2]),
                (x_, u, xR1, np.zeros((2, H, 3, 6)))):
        with pytest.raises(ValueError, match="shapes"):
            h.clearance_mesh_motion(*bad)
    assert len(h._lib.calls) == n


@pytest.mark.parametrize("cls", ["CFS_FANUC", "PSGCFS_FANUC"])
def test_solver_classes_attach_the_audit_and_audit_mesh_with_a_pose_still_raises(cls, monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    P = M.poses_z(s.H, -0.3, 0.6)
    cell = obs + [dict(mesh=_mesh(), epsilon=0.25, D=0.2, pose=P)]
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="audit_mesh"):
        getattr(pkg, cls)(cell, s, R, audit_mesh=8)
    with pytest.raises(ValueError, match="audit_mesh"):
        getattr(pkg, cls)(cell, s, R, audit_mesh=8, audit_mesh_motion=8)
    for bad in (0, 65, -3, 8.0, "8", True):
        with pytest.raises(ValueError, match="audit_mesh_motion"):
            getattr(pkg, cls)(cell, s, R, audit_mesh_motion=bad)
    with pytest.raises(ValueError, match="audit_mesh_motion"):
        getattr(pkg, cls)(obs, s, R, audit_mesh_motion=8)                 # no mesh in the cell
    assert not touched
    # the audit is taken after the solve, on the solve's outputs, with the option's S
    audits = []
    r = SimpleNamespace(u=np.zeros((1, s.H * 5)), x_=np.ones((1, s.H * 10)), iter_O=np.array([2]), total_iter=np.array([3]),
                        status=np.array([0]), cost_all=np.zeros((1, 4)), e_cost_all=np.zeros((1, 4)), e_u_all=np.zeros((1, 4)),
                        viol_all=np.zeros((1, 4)), n_soft=np.zeros(1, int))
    res = SimpleNamespace(dist_path=np.full((1, 2), 0.1), short_by=np.array([0.15]))

    def audit(x_, u, xR1, ob, substeps):
        audits.append((x_, u, substeps))
        return res

    stub = SimpleNamespace(set_meshes=lambda m: None, set_mesh_motion=lambda p: None, solve=lambda *a, **k: r,
                           clearance_mesh_motion=audit, clearance_mesh=lambda *a, **k: pytest.fail("the static audit was called"))
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: stub)
    a = getattr(pkg, cls)(cell, s, R)
    assert a.audit_mesh_motion is None and a.clearance_mesh_motion is None
    a.optimizer()
    assert a.clearance_mesh_motion is None and not audits
    b = getattr(pkg, cls)(cell, s, R, audit_mesh_motion=12).optimizer()
    assert len(audits) == 1 and audits[0][0] is r.x_ and audits[0][1] is r.u and audits[0][2] == 12
    assert b.clearance_mesh_motion.short_by == 0.15 and b.clearance_mesh_motion.dist_path.shape == (2,)
    assert b.clearance_mesh is None and b.clearance is None


def test_chomp_refuses_the_new_argument(monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    cell = [dict(num_obs=len(obs))] + [dict(o) for o in obs]
    with pytest.raises(ValueError, match="audit_mesh_motion"):
        pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit_mesh_motion=8)
    assert not touched
    pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit_mesh_motion=None)
    assert touched == [1]
