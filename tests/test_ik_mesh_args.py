"""Inverse kinematics against mesh obstacles: the entry points exist and are bound, and every refusal of IKSolver, of
plan_to_pose(ik_meshes=...) and of the C entry points themselves happens before the device is touched.  No compute calls here (CPU)."""
import ctypes as C

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from test_ik_args import LINE, ROBOT, _Stub, _desc


def _mesh():
    """a Mesh object without a handle: enough for the checks that run before the library is asked"""
    m = pkg.Mesh.__new__(pkg.Mesh)
    m._h = None
    return m


def test_entry_points_are_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ("cfs_ik_solve_mesh", "cfs_ik_solve_mesh_device", "cfs_debug_ik_frontier_overflows"):
        assert hasattr(h, n) and n in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                               # purely additive
    assert _lib.IK_MESH == _lib.RRT_MESH == {"per_lane": 1, "wave": 2, "small_frontier": 4}


@pytest.mark.parametrize("obs,kw", [
    ([dict(mesh=_mesh(), D=0.1), LINE], {}),                              # a mesh before a line
    ([LINE, dict(mesh=_mesh(), D=0.0)], {}), ([LINE, dict(mesh=_mesh(), D=-0.1)], {}), ([LINE, dict(mesh=_mesh(), D=float("nan"))], {}),
    ([LINE, dict(mesh=_mesh(), D=float("inf"))], {}), ([LINE, dict(mesh=_mesh(), D=True)], {}), ([LINE, dict(mesh=_mesh(), D="wide")], {}),
    ([LINE, dict(mesh=_mesh())], {}),
    ([LINE, dict(mesh=_mesh(), D=0.1)], dict(mesh_variant="fast")), ([LINE, dict(mesh=_mesh(), D=0.1)], dict(mesh_variant=2)),
    ([LINE], dict(mesh_variant="fast")),
    ([LINE, dict(mesh=object(), D=0.1)], {}), ([dict(mesh=np.zeros((2, 3, 3)), D=0.1)], {}),      # not a Mesh
    ([LINE] * 32 + [dict(mesh=_mesh(), D=0.1)], {}),
])
def test_solver_arguments_are_validated(obs, kw):
    with pytest.raises(ValueError):
        pkg.IKSolver(ROBOT, obs, **kw)


def test_a_well_formed_cell_is_accepted_without_a_device():
    m = _mesh()
    slv = pkg.IKSolver(ROBOT, [LINE, dict(mesh=m, D=0.1)], mesh_variant="per_lane")
    assert slv.obs.shape == (1, 6) and slv._meshes == [m] and slv._D_mesh.tolist() == [0.1] and slv.mesh_variant == "per_lane"
    assert slv._desc(True, 0, slv.obs, slv.D).nobs == 1                   # the descriptor holds the lines only
    assert pkg.IKSolver(ROBOT, [LINE])._meshes == []


@pytest.mark.parametrize("bad", [1, 0, None, "yes", np.bool_(True)])
def test_plan_to_pose_refuses_a_non_bool_ik_meshes(bad):
    with pytest.raises(ValueError, match="ik_meshes"):
        _Stub().plan_to_pose(np.zeros(5), np.zeros(3), ik_meshes=bad)
    with pytest.raises(ValueError, match="ik_meshes"):
        _Stub(meshes=[object()]).plan_to_pose(np.zeros(5), np.zeros(3), ik_meshes=bad)


def test_plan_to_pose_names_the_keyword_when_it_refuses_a_mesh_planner():
    with pytest.raises(ValueError, match="ik_meshes=True"):
        _Stub(meshes=[object()]).plan_to_pose(np.zeros(5), np.zeros(3))


def test_c_entry_points_refuse_bad_mesh_arguments_and_write_nothing():
    lib = pkg.lib()
    slv, d, o, z, zi = _desc()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tp, tr = np.ones((2, 3)), np.zeros((2, 5))
    fake = np.zeros(64, np.int64)                                        # an empty mesh of device 0: no triangles, nothing to read
    arr = (C.c_void_p * 2)(fake.ctypes.data, fake.ctypes.data)
    Dm = np.array([0.1, 0.2])

    def call(nmesh=2, meshes=arr, D=Dm, flags=0, T=2, out=o, dev=False):
        if dev:
            return lib.cfs_ik_solve_mesh_device(C.byref(d), nmesh, meshes, None if D is None else p(D), flags, T, p(tp), p(tp), p(tr), C.byref(out), None)
        return lib.cfs_ik_solve_mesh(C.byref(d), nmesh, meshes, None if D is None else p(D), flags, T, p(tp), p(tp), p(tr), C.byref(out))
    if pkg.device_count() == 0:
        assert call() == -2                                              # well formed: no device (never a CPU fallback)
    z[:] = 7.0
    zi[:] = 7

    def refused(**kw):
        for dev in (False, True):
            assert call(dev=dev, **kw) == -1 and lib.cfs_last_error(), kw
            assert (z == 7.0).all() and (zi == 7).all()                  # nothing written
    refused(nmesh=0)
    refused(nmesh=-1)
    refused(meshes=None)
    refused(meshes=(C.c_void_p * 2)(fake.ctypes.data, None))             # a NULL entry
    refused(D=None)
    for bad in (0.0, -0.1, np.nan, np.inf):
        refused(D=np.array([0.1, bad]))
    for flags in (8, 16, -1, 1 | 2, 1 | 4):                              # unknown bits; both variants; A with B's small frontier
        refused(flags=flags)
    keep = d.nobs
    many = (C.c_void_p * 32)(*[fake.ctypes.data] * 32)
    refused(nmesh=32, meshes=many, D=np.full(32, 0.1))                    # nobs + nmesh > CFS_MAX_OBS
    for field, bad in (("njoint", 7), ("restarts", 65), ("tol_pos", 0.0), ("nobs", 33)):      # everything cfs_ik_solve refuses
        k = getattr(d, field)
        setattr(d, field, bad)
        refused()
        setattr(d, field, k)
    assert d.nobs == keep
    refused(T=0)
    refused(out=_lib.cfs_ik_out())
    n = C.c_ulonglong(0)
    assert lib.cfs_debug_ik_frontier_overflows(None, 0) == -1
    assert lib.cfs_debug_ik_frontier_overflows(C.byref(n), 0) in (0, -2)
