"""Joint position limits at the Python surface and at the C setter's argument checks, without a device (CPU): malformed limits are
refused before anything reaches the library, and robotproperty2 carries the reference's joint ranges."""
import ctypes as C

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib, solvers


def test_thetamax_is_the_reference_literals():
    # robotproperty2.m:18-19 (degrees .* pi/180), :62, :106
    deg = np.array([[-170, 170], [-100, 145], [-72, 240], [-190, 190], [-125, 125], [-360, 360]])
    np.testing.assert_array_equal(pkg.robotproperty2("M200i").thetamax, deg * np.pi / 180)
    np.testing.assert_array_equal(pkg.robotproperty2("M16iB").thetamax,
                                  [[-np.pi, np.pi], [0, np.pi], [-np.pi, np.pi], [-np.pi, np.pi], [-np.pi / 2, np.pi / 2], [-np.pi, np.pi]])
    np.testing.assert_array_equal(pkg.robotproperty2("2L").thetamax, [[-np.pi, np.pi], [-np.pi, np.pi]])
    for rid in ("M200i", "M16iB", "2L"):
        r = pkg.robotproperty2(rid)
        assert r.thetamax.shape == (r.nlink if rid != "2L" else 2, 2)


def test_joint_limits_array_forms():
    robot = pkg.robotproperty2("M200i")
    assert solvers._joint_limits_array(None, robot, 5) is None
    np.testing.assert_array_equal(solvers._joint_limits_array("robot", robot, 5), robot.thetamax[:5])
    a = solvers._joint_limits_array([[-1, 1]] * 4 + [[-np.inf, np.inf]], robot, 5)
    assert a.shape == (5, 2) and a.dtype == np.float64 and np.isinf(a[4]).all()


@pytest.mark.parametrize("bad", [
    "cell", [[-1, 1]] * 4, np.zeros((5, 3)), [[-1, 1]] * 4 + [[np.nan, 1]], [[-1, 1]] * 4 + [[1, 1]], [[-1, 1]] * 4 + [[2, 1]],
    [[-1, 1]] * 4 + [[np.inf, np.inf]], [["a", "b"]] * 5,
], ids=["string", "rows", "cols", "nan", "equal", "reversed", "inf-inf", "text"])
def test_malformed_limits_are_refused_before_the_device(bad):
    R, s, obs = pkg.main_FANUC_problem()
    with pytest.raises(ValueError):
        pkg.CFSBatch(s, 2, [0.25, 0.25], joint_limits=bad)
    with pytest.raises(ValueError):
        pkg.CFS_FANUC(obs, s, R, joint_limits=bad)
    with pytest.raises(ValueError):
        pkg.PSGCFS_FANUC(obs, s, R, joint_limits=bad)


def test_robot_without_thetamax_is_refused():
    from types import SimpleNamespace
    robot = SimpleNamespace(name="custom")
    with pytest.raises(ValueError):
        solvers._joint_limits_array("robot", robot, 5)


def test_c_setter_refuses_a_null_handle():
    lib = _lib.lib()
    lo, hi = np.full(5, -1.0), np.full(5, 1.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cfs_problem_set_joint_limits(None, p(lo), p(hi)) == -1
    assert lib.cfs_problem_set_joint_limits(None, None, None) == -1
    on = C.c_int(7)
    assert lib.cfs_problem_get_joint_limits(None, C.byref(on), p(lo), p(hi)) == -1
    assert "NULL" in lib.cfs_last_error().decode()


def test_header_documents_the_entry_points():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfs_hip.h")).read()
    assert "int cfs_problem_set_joint_limits(cfs_problem *p, const double *lo, const double *hi);" in hdr
    assert "int cfs_problem_get_joint_limits(const cfs_problem *p, int *on, double *lo, double *hi);" in hdr
