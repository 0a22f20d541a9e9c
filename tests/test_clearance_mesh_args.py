"""The mesh clearance audit's entry points exist, are bound, and every Python surface (CFSBatch.clearance_mesh /
clearance_mesh_device, the audit_mesh= option of the solver classes) refuses bad arguments before anything touches the device.
No compute calls here (CPU)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("cfs_clearance_mesh", "cfs_clearance_mesh_device"):
        assert hasattr(h, n) and n in names
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive
    src = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "cfs_clearance_mesh_device" in src and "1-Lipschitz" in src and "tri_path" in src
    assert _lib.DBG["clear_no_bound"] == 256 and _lib.DBG["clear_seed"] == 512
    assert "#define CFS_DBG_CLEAR_NO_BOUND 256" in src and "#define CFS_DBG_CLEAR_SEED 512" in src


def test_null_handle_is_refused():
    lib = pkg.lib()
    z = np.zeros(64)
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.cfs_clearance_mesh(None, 1, 16, p, p, p, p, p, p, p, p, p, p) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert lib.cfs_clearance_mesh_device(None, 1, 16, p, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert (z == 0).all()                                                # nothing written


class _NoDevice:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


class _Handle(pkg.CFSBatch):
    """a CFSBatch with the shape of config 3 and no handle behind it (the argument checks come before the library)"""
    obstacle_motion = "static"

    def __init__(self, meshes=(object(),)):
        self.H, self.nj, self.ns, self.nn, self.nx, self.nobs, self.max_batch = 30, 5, 10, 150, 300, 8, 4
        self.margin = np.full(8, 0.2)
        self._lib, self._h, self._meshes = _NoDevice(), None, list(meshes)

    def close(self):
        pass

    __del__ = close


def _arrays(B=2):
    return np.zeros((B, 300)), np.zeros((B, 150)), np.zeros((B, 10)), np.zeros((B, 8, 6))


@pytest.mark.parametrize("S", [0, -1, 65, 1000, 16.0, "16", None, True, np.nan])
def test_bad_substeps_are_refused(S):
    with pytest.raises(ValueError, match="substeps"):
        _Handle().clearance_mesh(*_arrays(), substeps=S)
    with pytest.raises(ValueError, match="substeps"):
        _Handle().clearance_mesh_device(*_arrays(), substeps=S)          # refused before the tensors are looked at


def test_handles_without_meshes_and_bad_shapes_are_refused():
    with pytest.raises(ValueError, match="mesh"):
        _Handle(meshes=[]).clearance_mesh(*_arrays())
    with pytest.raises(ValueError, match="mesh"):
        _Handle(meshes=[]).clearance_mesh_device(*_arrays())
    h = _Handle()
    del h._meshes                                                        # set_meshes was never called
    with pytest.raises(ValueError, match="mesh"):
        h.clearance_mesh(*_arrays())
    x_, u, xR1, obs = _arrays()
    for bad in ((x_[:, :-1], u, xR1, obs), (x_, u[:1], xR1, obs), (x_, u, xR1[:, :5], obs), (x_, u, xR1, obs[:, :7]),
                (x_, u, xR1, np.zeros((2, 30, 8, 6)))):
        with pytest.raises(ValueError, match="shapes"):
            _Handle().clearance_mesh(*bad)


@pytest.mark.parametrize("cls", ["CFS_FANUC", "PSGCFS_FANUC"])
@pytest.mark.parametrize("audit_mesh", [0, 65, -3, 8.0, "8", True])
def test_solver_classes_validate_audit_mesh_before_the_device(cls, audit_mesh, monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="audit_mesh"):
        getattr(pkg, cls)(obs + [dict(mesh=object(), epsilon=0.1, D=0.1)], s, R, audit_mesh=audit_mesh)
    assert not touched


def test_audit_mesh_needs_a_mesh_audit_keeps_refusing_them_and_chomp_refuses_audit_mesh(monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="audit_mesh"):
        pkg.CFS_FANUC(obs, s, R, audit_mesh=8)                           # line obstacles only: that is audit='s job
    with pytest.raises(ValueError, match="mesh"):
        pkg.PSGCFS_FANUC(obs + [dict(mesh=object(), epsilon=0.1, D=0.1)], s, R, audit=8, audit_mesh=8)
    cell = [dict(num_obs=len(obs))] + [dict(o) for o in obs]
    with pytest.raises(ValueError, match="audit_mesh"):
        pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit_mesh=8)
    assert not touched
    pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit_mesh=None)   # None is the default everywhere
    assert touched == [1]


def test_audit_mesh_default_leaves_the_solver_object_as_it_was(monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    cell = obs + [dict(mesh=object(), epsilon=0.25, D=0.2)]
    made = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: made.append((a, k)) or SimpleNamespace(set_meshes=lambda m: None))
    a = pkg.CFS_FANUC(cell, s, R)
    b = pkg.CFS_FANUC(cell, s, R, audit_mesh=16)
    assert a.audit_mesh is None and a.clearance_mesh is None and a.audit is None and a.clearance is None
    assert b.audit_mesh == 16 and b.clearance_mesh is None and b.audit is None
    assert made[0][1] == made[1][1]                                      # the handle is created with the same options
