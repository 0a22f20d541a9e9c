"""The clearance audit's entry points exist, are bound, and every Python surface (CFSBatch.clearance / clearance_device, the
audit= option of the solver classes, min_clearance= / audit_substeps= of RRTCFSPlanner) refuses bad arguments before anything
touches the device.  No compute calls here (CPU)."""
import ctypes as C
import math
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
    for n in ("cfs_clearance", "cfs_clearance_device"):
        assert hasattr(h, n) and n in names
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive
    src = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "cfs_clearance_device" in src and "Lib/CFS_FANUC.m:110-120" in src and "robotproperty2.m:136-139" in src


def test_null_handle_is_refused():
    lib = pkg.lib()
    z = np.zeros(64)
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.cfs_clearance(None, 1, 16, p, p, p, p, p, p, p, p, p) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert lib.cfs_clearance_device(None, 1, 16, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert (z == 0).all()                                                # nothing written


class _NoDevice:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


class _Handle(pkg.CFSBatch):
    """a CFSBatch with the shape of config 3 and no handle behind it (the argument checks come before the library)"""
    obstacle_motion = "static"

    def __init__(self, meshes=(), motion="static"):
        self.H, self.nj, self.ns, self.nn, self.nx, self.nobs, self.max_batch = 30, 5, 10, 150, 300, 8, 4
        self.margin = np.full(8, 0.2)
        self._lib, self._h, self._meshes, self.obstacle_motion = _NoDevice(), None, list(meshes), motion

    def close(self):
        pass

    __del__ = close


_handle = _Handle


def _arrays(B=2, H=None):
    obs = np.zeros((B, 8, 6)) if H is None else np.zeros((B, H, 8, 6))
    return np.zeros((B, 300)), np.zeros((B, 150)), np.zeros((B, 10)), obs


@pytest.mark.parametrize("S", [0, -1, 65, 1000, 16.0, "16", None, True, np.nan])
def test_bad_substeps_are_refused(S):
    with pytest.raises(ValueError, match="substeps"):
        _handle().clearance(*_arrays(), substeps=S)
    with pytest.raises(ValueError, match="substeps"):
        _handle().clearance_device(*_arrays(), substeps=S)               # refused before the tensors are looked at


def test_mesh_handles_and_bad_shapes_are_refused():
    with pytest.raises(ValueError, match="mesh"):
        _handle(meshes=[object()]).clearance(*_arrays())
    with pytest.raises(ValueError, match="mesh"):
        _handle(meshes=[object()]).clearance_device(*_arrays())
    x_, u, xR1, obs = _arrays()
    with pytest.raises(ValueError, match="shapes"):
        _handle().clearance(x_[:, :-1], u, xR1, obs)
    with pytest.raises(ValueError, match="shapes"):
        _handle().clearance(x_, u[:1], xR1, obs)
    with pytest.raises(ValueError, match="shapes"):
        _handle().clearance(x_, u, xR1[:, :5], obs)
    with pytest.raises(ValueError, match="per-waypoint"):
        _handle(motion="per_waypoint").clearance(x_, u, xR1, obs)        # a per-waypoint handle takes (B, H, nobs, 6)
    with pytest.raises(AssertionError):
        _handle().clearance(*_arrays(H=30))                              # and a static one (B, nobs, 6), as every other entry


@pytest.mark.parametrize("cls", ["CFS_FANUC", "PSGCFS_FANUC"])
@pytest.mark.parametrize("audit", [0, 65, -3, 8.0, "8", True])
def test_solver_classes_validate_audit_before_the_device(cls, audit, monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="audit"):
        getattr(pkg, cls)(obs, s, R, audit=audit)
    assert not touched


def test_audit_refuses_mesh_obstacles_and_chomp_refuses_audit(monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    touched = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="mesh"):
        pkg.CFS_FANUC(obs + [dict(mesh=object(), epsilon=0.1, D=0.1)], s, R, audit=8)
    cell = [dict(num_obs=len(obs))] + [dict(o) for o in obs]
    with pytest.raises(ValueError, match="audit"):
        pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit=8)
    assert not touched
    pkg.CHOMP_FANUC(cell, s, np.zeros(s.H * s.nu), R, audit=None)          # None is the default everywhere
    assert touched == [1]


def test_audit_default_leaves_the_solver_object_as_it_was(monkeypatch):
    R, s, obs = pkg.main_FANUC_problem()
    made = []
    monkeypatch.setattr(solvers, "CFSBatch", lambda *a, **k: made.append((a, k)) or SimpleNamespace(set_meshes=lambda m: None))
    a = pkg.CFS_FANUC(obs, s, R)
    b = pkg.CFS_FANUC(obs, s, R, audit=16)
    assert a.audit is None and a.clearance is None and b.audit == 16
    assert made[0][1] == made[1][1]                                      # the handle is created with the same options


@pytest.mark.parametrize("kw", [dict(min_clearance=-0.01), dict(min_clearance=math.nan), dict(min_clearance=math.inf),
                                dict(min_clearance="0.02"), dict(min_clearance=True), dict(audit_substeps=0),
                                dict(audit_substeps=65), dict(audit_substeps=8.0), dict(min_clearance=0.02, audit_substeps=None)])
def test_planner_validates_the_audit_options_before_the_device(kw, monkeypatch):
    pobs, s, g, region_g, region_s, off = pkg.RRTstar_problem()
    touched = []
    monkeypatch.setattr(pkg.plan, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError):
        pkg.RRTCFSPlanner(pobs, s, region_g, region_s, off, **kw)
    assert not touched
