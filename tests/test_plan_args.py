"""cfs_select_best_device and RRTCFSPlanner: the entry point exists, is bound, and refuses bad arguments before the device;
the planner validates its arguments before it creates a handle.  No compute calls here (CPU)."""
import ctypes as C
import math

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib


def test_entry_point_is_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    assert hasattr(h, "cfs_select_best_device")
    assert "cfs_select_best_device" in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                              # purely additive
    assert pkg.RRTCFSPlanner is pkg.plan.RRTCFSPlanner and "RRTCFSPlanner" in pkg.__all__


def _args():
    z = np.zeros(64)
    p = z.ctypes.data_as(C.c_void_p)
    o = _lib.cfs_batch_out()
    for k, _ in _lib.cfs_batch_out._fields_:
        setattr(o, k, p)
    return z, p, o


@pytest.mark.parametrize("K", [0, -1, 65, 1000])
def test_K_outside_1_to_64_is_refused(K):
    lib = pkg.lib()
    z, p, o = _args()
    assert lib.cfs_select_best_device(None, 1, K, p, C.byref(o), None, C.byref(o), None, p, p, None) == -1
    assert f"K={K}".encode() in lib.cfs_last_error()


def test_null_handle_and_null_arrays_are_refused():
    lib = pkg.lib()
    z, p, o = _args()
    assert lib.cfs_select_best_device(None, 1, 6, p, C.byref(o), None, C.byref(o), None, p, p, None) == -1
    assert b"NULL handle" in lib.cfs_last_error()
    assert lib.cfs_select_best_device(None, 0, 6, p, C.byref(o), None, C.byref(o), None, p, p, None) == -1
    assert b"S=0" in lib.cfs_last_error()
    fake = C.c_void_p(1)                                                   # never dereferenced: the NULL checks come first
    for i in range(5):
        a = [p, C.byref(o), C.byref(o), p, p]
        a[i] = None
        rc = lib.cfs_select_best_device(fake, 1, 6, a[0], a[1], None, a[2], None, a[3], a[4], None)
        assert rc == -1 and b"NULL argument" in lib.cfs_last_error()
    for field, _ in _lib.cfs_batch_out._fields_:
        bad = _lib.cfs_batch_out()
        C.memmove(C.byref(bad), C.byref(o), C.sizeof(o))
        setattr(bad, field, None)
        assert lib.cfs_select_best_device(fake, 1, 6, p, C.byref(bad), None, C.byref(o), None, p, p, None) == -1
        assert lib.cfs_select_best_device(fake, 1, 6, p, C.byref(o), None, C.byref(bad), None, p, p, None) == -1
        assert b"NULL array" in lib.cfs_last_error()
    assert lib.cfs_select_best_device(fake, 1, 6, p, C.byref(o), None, C.byref(o), p, p, p, None) == -1
    assert b"best_viol_all needs cand_viol_all" in lib.cfs_last_error()


def _problem():
    return pkg.RRTstar_problem()          # pobs, sys_rrt, goal, region_g, region_s, sample_off


@pytest.mark.parametrize("kw", [dict(select="fewest"), dict(select=None), dict(num_seed=0), dict(num_seed=65), dict(num_seed=6.0),
                                dict(num_seed=True), dict(max_slots=0), dict(max_slots=2.5), dict(mode="CHOMP"),
                                dict(rrt_solver="PRM"), dict(ROBOT="M16iB"), dict(jacobian="exact"),
                                dict(on_infeasible="soften"), dict(on_infeasible="soften", soft_weight=-1.0),
                                dict(on_infeasible="soften", soft_weight=math.nan), dict(on_infeasible="never"),
                                dict(device="cpu")])
def test_planner_arguments_are_validated_before_the_device(kw, monkeypatch):
    pobs, s, g, region_g, region_s, off = _problem()
    touched = []
    monkeypatch.setattr(pkg.plan, "CFSBatch", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError):
        pkg.RRTCFSPlanner(pobs, s, region_g, region_s, off, **kw)
    assert not touched                                                    # no handle was asked for


class _Stub(pkg.RRTCFSPlanner):
    """the planner's plan() argument checks without a handle (they run before any GPU call)"""

    def __init__(self, K=6, max_slots=4):
        import torch
        self.K, self.max_slots, self.nj, self.device = K, max_slots, 5, torch.device("cuda", 0)

    def _plan(self, *a):
        raise AssertionError("reached the device")


@pytest.mark.parametrize("x0,goal,kw", [
    (np.zeros(4), np.zeros(5), {}),                      # wrong joint count
    (np.zeros((2, 5)), np.zeros((3, 5)), {}),            # S disagrees
    (np.zeros((5, 5)), np.zeros(5), {}),                 # S > max_slots
    (np.zeros((0, 5)), np.zeros(5), {}),                 # no slot
    (np.zeros((1, 2, 5)), np.zeros(5), {}),              # rank 3
    (np.full(5, np.nan), np.zeros(5), {}),               # not finite
    (np.zeros(5), np.zeros(5), dict(seed=-1)),
    (np.zeros(5), np.zeros(5), dict(seed=1.5)),
    (np.zeros(5), np.zeros(5), dict(max_rounds=0)),
    (np.zeros(5), np.zeros(5), dict(max_draws=0)),
    (np.zeros(5), np.zeros(5), dict(timings=[])),
])
def test_plan_arguments_are_validated_before_the_device(x0, goal, kw):
    kw = dict(dict(seed=1), **kw)
    with pytest.raises(ValueError):
        _Stub().plan(x0, goal, **kw)


def test_plan_refuses_tensors_on_another_device():
    import torch
    with pytest.raises(ValueError):
        _Stub().plan(torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.float64), seed=1)
