"""The Jacobian-mode entry points (cfs_problem_set_jacobian / cfs_problem_get_jacobian / cfs_dist_arm_grad) and the Python
jacobian= argument: they exist, and refuse NULL handles, unknown modes and malformed arguments before touching the device.
No compute calls here (CPU)."""
import ctypes as C

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib


def test_entry_points_are_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ("cfs_problem_set_jacobian", "cfs_problem_get_jacobian", "cfs_dist_arm_grad"):
        assert hasattr(h, n)
        assert n in [s[0] for s in _lib.SYMBOLS]
    assert _lib.JACOBIAN == {"fd_literal": 0, "analytic": 1}
    assert pkg.lib().cfs_abi_version() == 1


def test_mode_entry_points_validate_before_the_device():
    lib = pkg.lib()
    m = C.c_int(7)
    assert lib.cfs_problem_set_jacobian(None, 0) == -1
    assert lib.cfs_problem_set_jacobian(None, 1) == -1
    assert lib.cfs_problem_get_jacobian(None, C.byref(m)) == -1
    assert m.value == 7                                              # nothing written on failure
    assert b"NULL" in lib.cfs_last_error()


def test_dist_arm_grad_validates_its_arguments():
    lib = pkg.lib()
    rb = pkg.to_c_robot(pkg.robotproperty2("M200i"))
    th, ob = np.zeros((3, 5)), np.zeros((2, 6))
    d, g = np.zeros((3, 2)), np.zeros((3, 2, 5))
    lid = np.zeros((3, 2), np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    assert lib.cfs_dist_arm_grad(None, 5, 3, P(th), 2, P(ob), P(d), P(lid), P(g)) == -1           # NULL robot
    assert lib.cfs_dist_arm_grad(C.byref(rb), 7, 3, P(th), 2, P(ob), P(d), P(lid), P(g)) == -1    # njoint out of range
    assert lib.cfs_dist_arm_grad(C.byref(rb), 5, -1, P(th), 2, P(ob), P(d), P(lid), P(g)) == -1   # negative N
    assert lib.cfs_dist_arm_grad(C.byref(rb), 5, 3, None, 2, P(ob), P(d), P(lid), P(g)) == -1     # NULL theta
    assert lib.cfs_dist_arm_grad(C.byref(rb), 5, 3, P(th), 2, P(ob), P(d), P(lid), None) == -1    # NULL grad
    assert lib.cfs_dist_arm_grad(C.byref(rb), 5, 3, P(th), 2, P(ob), P(d), None, P(g)) == -1      # NULL linkid
    r2 = pkg.to_c_robot(pkg.robotproperty2("2L"))
    assert lib.cfs_dist_arm_grad(C.byref(r2), 3, 3, P(th), 2, P(ob), P(d), P(lid), P(g)) == -1    # the 2L model has 2 joints
    if pkg.device_count() == 0:
        assert lib.cfs_dist_arm_grad(C.byref(rb), 5, 3, P(th), 2, P(ob), P(d), P(lid), P(g)) == -2   # CFS_ERR_NO_DEVICE
        with pytest.raises(pkg.CfsError) as e:
            pkg.dist_arm(pkg.robotproperty2("M200i"), th, ob, want_grad=True)
        assert e.value.code == -2


def test_python_jacobian_argument_is_validated():
    R, s, obs = pkg.main_FANUC_problem()
    for bad in ("FD_LITERAL", "numeric", "", None, 1):
        with pytest.raises(ValueError):
            pkg.CFSBatch(s, 1, [0.25], jacobian=bad)
        with pytest.raises(ValueError):
            pkg.CFS_FANUC(obs, s, R, jacobian=bad)
        with pytest.raises(ValueError):
            pkg.PSGCFS_FANUC(obs, s, R, jacobian=bad)
    if pkg.device_count() == 0:                                       # a valid string goes on to the device (and finds none)
        with pytest.raises(pkg.CfsError) as e:
            pkg.CFS_FANUC(obs, s, R, jacobian="analytic")
        assert e.value.code == -2
