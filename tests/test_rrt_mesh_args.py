"""cfs_rrt_grow_mesh* and the Python layers above them refuse bad arguments before the device is touched: the C entries return
CFS_ERR_INVALID_ARG with nothing launched (this machine may have no GPU at all), RRT_FANUC and RRTCFSPlanner raise ValueError before
any library call.  No compute calls here (CPU)."""
import ctypes as C
import math

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from motionplanning_5d_m_amd.robotproperty2 import to_c_robot


def test_entry_points_are_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("cfs_rrt_grow_mesh", "cfs_rrt_grow_mesh_device", "cfs_debug_rrt_frontier_overflows"):
        assert hasattr(h, n) and n in names
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive


class _FakeMesh:
    """memory laid out like the head of a cfs_mesh (int device first); the argument checks read nothing else"""

    def __init__(self, device=0):
        self.buf = (C.c_int * 64)()
        self.buf[0] = device
        self._h = C.c_void_p(C.addressof(self.buf))


def _desc(max_iter=400, nobs=1):
    pobs, s, g, region_g, region_s, off = pkg.RRTstar_problem()
    keep = [np.ascontiguousarray(v, float) for v in (s.x0, g, g, region_g, region_s, off, s.ratial, np.zeros((max(nobs, 1), 6)), np.full(max(nobs, 1), 0.2))]
    d = _lib.cfs_rrt_desc()
    d.robot = to_c_robot(s.robot)
    d.nstate, d.solver, d.max_iter, d.bi, d.rewire, d.per_tree = 5, 0, max_iter, 0.5, 0.2, 0
    for k, v in zip(("x0", "goal", "goal_th", "region_g", "region_s", "sample_off", "ratial", "obs", "D"), keep):
        setattr(d, k, v.ctypes.data_as(C.c_void_p))
    d.nobs, d.seed, d.max_draws = nobs, 1, 1000
    z = np.zeros(8 * 1024)
    o = _lib.cfs_rrt_out()
    for k in ("node_num", "fail", "parent", "nodes", "total_dis", "route_len", "route"):
        setattr(o, k, z.ctypes.data_as(C.c_void_p))
    return d, o, (keep, z)


def _call(d, nmesh, meshes, D, flags, o, device_entry):
    lib = pkg.lib()
    arr = None if meshes is None else (C.c_void_p * max(len(meshes), 1))(*[None if m is None else m._h for m in meshes])
    Dm = None if D is None else np.ascontiguousarray(D, float)
    Dp = None if Dm is None else Dm.ctypes.data_as(C.c_void_p)
    if device_entry:
        rc = lib.cfs_rrt_grow_mesh_device(C.byref(d), nmesh, arr, Dp, flags, 1, C.byref(o), None)
    else:
        rc = lib.cfs_rrt_grow_mesh(C.byref(d), nmesh, arr, Dp, flags, 1, C.byref(o))
    return rc, lib.cfs_last_error()


@pytest.mark.parametrize("device_entry", [False, True])
def test_c_entries_refuse_bad_mesh_arguments_before_the_device(device_entry):
    d, o, keep = _desc()
    m = _FakeMesh()
    cases = [
        (dict(nmesh=-1, meshes=[m], D=[0.1]), b"nmesh"),
        (dict(nmesh=1, meshes=None, D=[0.1]), b"must be given"),
        (dict(nmesh=1, meshes=[m], D=None), b"must be given"),
        (dict(nmesh=2, meshes=[m, None], D=[0.1, 0.1]), b"is NULL"),
        (dict(nmesh=1, meshes=[_FakeMesh(device=5)], D=[0.1]), b"lives on device 5"),
        (dict(nmesh=1, meshes=[m], D=[0.0]), b"finite and > 0"),
        (dict(nmesh=1, meshes=[m], D=[-0.1]), b"finite and > 0"),
        (dict(nmesh=1, meshes=[m], D=[math.nan]), b"finite and > 0"),
        (dict(nmesh=1, meshes=[m], D=[math.inf]), b"finite and > 0"),
        (dict(nmesh=1, meshes=[m], D=[0.1], flags=8), b"unknown flags"),
        (dict(nmesh=1, meshes=[m], D=[0.1], flags=-1), b"unknown flags"),
        (dict(nmesh=1, meshes=[m], D=[0.1], flags=3), b"excludes"),
        (dict(nmesh=0, meshes=None, D=None, flags=64), b"unknown flags"),
    ]
    for kw, msg in cases:
        rc, err = _call(d, kw["nmesh"], kw["meshes"], kw["D"], kw.get("flags", 0), o, device_entry)
        assert rc == -1 and msg in err, (kw, rc, err)
    # nobs + nmesh > CFS_MAX_OBS
    d2, o2, keep2 = _desc(nobs=1)
    many = [m] * _lib.CFS_MAX_OBS
    rc, err = _call(d2, len(many), many, [0.1] * len(many), 0, o2, device_entry)
    assert rc == -1 and b"nmesh" in err
    # every refusal of cfs_rrt_grow still holds
    d3, o3, keep3 = _desc()
    d3.solver = 7
    rc, err = _call(d3, 1, [m], [0.1], 0, o3, device_entry)
    assert rc == -1 and b"unknown solver" in err
    d3, o3, keep3 = _desc()
    o3.route = None
    rc, err = _call(d3, 1, [m], [0.1], 0, o3, device_entry)
    assert rc == -1 and b"NULL output array" in err


def test_null_descriptor_is_refused():
    lib = pkg.lib()
    assert lib.cfs_debug_rrt_frontier_overflows(None, 0) == -1 and b"nothing to do" in lib.cfs_last_error()
    o = _lib.cfs_rrt_out()
    assert lib.cfs_rrt_grow_mesh(None, 0, None, None, 0, 1, C.byref(o)) == -1
    assert b"NULL descriptor" in lib.cfs_last_error()


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_max_iter_that_no_longer_fits_next_to_the_mesh_scratch_is_refused(flags):
    """MAX_ITER = 1000 fits the line-only kernel's 64 KB (61 064 B) but not with the 10 KB of traversal stacks behind the tree"""
    d, o, keep = _desc(max_iter=1000)
    rc, err = _call(d, 1, [_FakeMesh()], [0.1], flags, o, True)
    assert rc == -1 and b"does not fit" in err, err
    d, o, keep = _desc(max_iter=1200)                                      # and what cfs_rrt_grow refuses stays refused
    rc, err = _call(d, 0, None, None, 0, o, True)
    assert rc == -1 and b"MAX_ITER" in err


# ---- Python layers --------------------------------------------------------------------------------------------------------------
class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def _cell(D=0.1, epsilon=0.15, first=False):
    pobs, s, g, region_g, region_s, off = pkg.RRTstar_problem()
    mesh = dict(mesh=_FakeMesh(), D=D, epsilon=epsilon)
    cell = [mesh, pobs[0]] if first else [pobs[0], mesh]
    return cell, s, g, region_g, region_s, off


@pytest.mark.parametrize("kw", [dict(first=True), dict(D=0.0), dict(D=-1.0), dict(D=math.nan), dict(D=math.inf)])
def test_rrt_fanuc_refuses_a_bad_cell_before_any_library_call(kw, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    cell, s, g, region_g, region_s, off = _cell(**kw)
    with pytest.raises(ValueError):
        pkg.RRT_FANUC(cell, s, g, region_g, region_s, off, "M200i", "RRT")


def test_rrt_fanuc_refuses_too_many_obstacles_and_bad_flags(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    cell, s, g, region_g, region_s, off = _cell()
    with pytest.raises(ValueError):
        pkg.RRT_FANUC([cell[0]] + [cell[1]] * _lib.CFS_MAX_OBS, s, g, region_g, region_s, off, "M200i", "RRT")
    planner = pkg.RRT_FANUC(cell, s, g, region_g, region_s, off, "M200i", "RRT")
    assert planner._obs_arr.shape == (1, 6) and planner._D.tolist() == [0.2] and planner._D_mesh.tolist() == [0.1]
    for bad in (8, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            planner.grow(seed=1, S=1, mesh_flags=bad)
    plain = pkg.RRT_FANUC(cell[:1], s, g, region_g, region_s, off, "M200i", "RRT")
    assert plain._meshes == [] and plain._obs_arr.shape == (1, 6)


@pytest.mark.parametrize("kw", [dict(first=True), dict(D=0.0), dict(epsilon=math.nan), dict(epsilon=-0.1),
                                dict(planner=dict(on_infeasible="soften", soft_weight=10.0)), dict(planner=dict(select="fewest"))])
def test_planner_refuses_a_bad_mesh_cell_before_the_device(kw, monkeypatch):
    pk = kw.pop("planner", {})
    cell, s, g, region_g, region_s, off = _cell(**kw)
    touched = []
    monkeypatch.setattr(pkg.plan, "CFSBatch", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    with pytest.raises(ValueError):
        pkg.RRTCFSPlanner(cell, s, region_g, region_s, off, **pk)
    assert not touched


def test_reference_map_workload_draws_what_config5_reference_map_draws():
    from motionplanning_5d_m_amd import workloads
    w = workloads.rrt_reference_map(S=8)
    s, bt, tri = workloads.config5_reference_map(B=8)
    np.testing.assert_array_equal(w.x0, bt.x0)
    np.testing.assert_array_equal(w.goal, bt.xg)
    np.testing.assert_array_equal(w.tri, tri)
    assert (w.D, w.epsilon) == (float(bt.margin_psg[0]), float(bt.margin_cfs[0])) == (0.2, 0.25)
    cell = w.obs_cell("m")
    assert cell == [dict(mesh="m", D=0.2, epsilon=0.25)] and w.sys_rrt.nstate == 5
