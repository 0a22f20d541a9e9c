"""Cartesian paths: the entry points exist and are bound, and every refusal of CartesianPath, of plan_to_pose's approach arguments
and of the C entry points themselves happens before the device is touched.  No compute calls here (CPU)."""
import ctypes as C

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib


def test_entry_points_are_exported_and_bound():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ("cfs_cart_path", "cfs_cart_path_device"):
        assert hasattr(h, n) and n in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                               # purely additive
    assert pkg.CartesianPath is pkg.cart.CartesianPath and {"CartesianPath", "cart"} <= set(pkg.__all__)
    assert _lib.CART_CAND_STATUS[4] == "JOINT_JUMP" and _lib.CART_STATUS[2] == "NO_START"


ROBOT = pkg.robotproperty2("M200i")
LINE = dict(l=np.array([[3.4, 3.4], [8.3, 8.3], [0.0, 1.2]]), D=0.1)


@pytest.mark.parametrize("kw", [
    dict(steps=0), dict(steps=257), dict(steps=8.0), dict(steps=True), dict(max_iter=0), dict(max_iter=1001), dict(max_iter=2.0),
    dict(max_joint_step=0.0), dict(max_joint_step=-0.1), dict(max_joint_step=float("nan")), dict(max_joint_step=float("inf")),
    dict(max_joint_step="small"), dict(max_joint_step=True),
    dict(tol_pos=0.0), dict(tol_pos=float("nan")), dict(tol_axis=float("inf")), dict(tol_axis="small"),
    dict(weight=[1, 1, 1, 1]), dict(weight=[1, 1, 1, 1, 0]), dict(weight=[1, 1, 1, 1, float("nan")]),
    dict(joint_limits=None), dict(joint_limits="cell"), dict(joint_limits=np.zeros((5, 2))), dict(joint_limits=np.array([[-1, np.inf]] * 5)),
    dict(tool=[0, 0]), dict(tool=[0, 0, float("nan")]), dict(tool_axis=[0, 0, 0]), dict(tool_axis=[0, float("inf"), 1]),
    dict(njoint=1), dict(njoint=7), dict(njoint=5.0), dict(device="cpu"),
    dict(obs=[dict(l=np.zeros((3, 3)), D=0.1)]), dict(obs=[dict(l=np.zeros((3, 2)), D=float("nan"))]), dict(obs=[LINE] * 33),
])
def test_solver_arguments_are_validated(kw):
    kw = dict(kw)
    obs = kw.pop("obs", [LINE])
    with pytest.raises(ValueError):
        pkg.CartesianPath(ROBOT, obs, **kw)


def test_mesh_obstacles_are_refused():
    class FakeMesh:
        pass
    with pytest.raises(ValueError, match="line obstacles only"):
        pkg.CartesianPath(ROBOT, [LINE, dict(mesh=FakeMesh(), D=0.1)])


def test_defaults():
    c = pkg.CartesianPath(ROBOT)
    assert (c.steps, c.max_iter, c.max_joint_step, c.tol_pos, c.tol_axis, c.nj) == (16, 20, 0.2, 1e-6, 1e-6, 5)
    np.testing.assert_array_equal(c.tool, ROBOT.cap[4].p[:, 0])
    np.testing.assert_array_equal(np.stack([c.lo, c.hi], axis=1), ROBOT.thetamax[:5])
    assert c.obs.shape == (0, 6) and c.weight is None
    assert pkg.CartesianPath(pkg.robotproperty2("M16iB")).nj == 6 and pkg.CartesianPath(pkg.robotproperty2("2L")).nj == 2


S1 = np.zeros((1, 4, 5))


@pytest.mark.parametrize("args,kw", [
    ((np.zeros(5), np.zeros(3)), {}), ((np.zeros((1, 4, 4)), np.zeros(3)), {}), ((np.zeros((1, 65, 5)), np.zeros(3)), {}),
    ((np.zeros((0, 4, 5)), np.zeros((0, 3))), {}), ((np.zeros((1, 0, 5)), np.zeros(3)), {}), (("here", np.zeros(3)), {}),
    ((np.zeros((2, 4, 5)), np.zeros((3, 3))), {}), ((S1, np.zeros(2)), {}), ((S1, np.full(3, np.nan)), {}), ((S1, np.zeros((2, 2, 3))), {}),
    ((S1, np.zeros(3), np.zeros(3)), {}), ((S1, np.zeros(3), [0, np.nan, 1]), {}), ((S1, np.zeros(3), np.ones((2, 3))), {}),
    ((S1, np.zeros(3), None, np.zeros(4)), {}), ((S1, np.zeros(3), None, np.full(5, np.inf)), {}),
    ((S1, np.zeros(3)), dict(start_state=np.zeros((1, 3), np.int32))), ((S1, np.zeros(3)), dict(start_state=np.zeros((1, 4)))),
    ((S1, np.zeros(3)), dict(start_state="all")),
])
def test_trace_arguments_are_validated_before_the_library(args, kw, monkeypatch):
    c = pkg.CartesianPath(ROBOT, [LINE])
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    with pytest.raises(ValueError):
        c.trace(*args, **kw)
    with pytest.raises(ValueError):
        c.trace_device(*args, **kw)                                       # host arrays are not CUDA tensors either


def _desc():
    c = pkg.CartesianPath(ROBOT, [LINE])
    d = c._desc(True, 4, c.obs, c.D)
    z = np.zeros(64)
    zi = np.zeros(64, np.int32)
    o = _lib.cfs_cart_out()
    o.theta, o.status = z.ctypes.data_as(C.c_void_p), zi.ctypes.data_as(C.c_void_p)
    return c, d, o, z, zi


def test_c_entry_points_refuse_bad_descriptors_and_write_nothing():
    lib = pkg.lib()
    c, d, o, z, zi = _desc()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st, ss, tp, tr = np.zeros((2, 4, 5)), np.zeros((2, 4), np.int32), np.ones((2, 3)), np.zeros((2, 5))
    call = lambda d_=d, T=2, s=st, s2=ss, a=tp, b=tp, r=tr, out=o: lib.cfs_cart_path(  # noqa: E731
        C.byref(d_) if d_ is not None else None, T, None if s is None else p(s), None if s2 is None else p(s2), None if a is None else p(a),
        None if b is None else p(b), None if r is None else p(r), C.byref(out) if out is not None else None)
    assert call() in (0, -2)                                              # well formed: runs, or no device (never a CPU fallback)
    assert call(s2=None) in (0, -2)                                       # start_state is optional
    if pkg.device_count() == 0:
        assert call() == -2 and b"device" in lib.cfs_last_error().lower()
    z[:] = 7.0
    zi[:] = 7

    def refused(**kw):
        assert call(**kw) == -1 and lib.cfs_last_error()
        assert (z == 7.0).all() and (zi == 7).all()                       # nothing written
    refused(d_=None)
    for field, bad in (("njoint", 1), ("njoint", 7), ("use_axis", 2), ("candidates", 0), ("candidates", 65), ("steps", 0), ("steps", 257),
                       ("max_iter", 0), ("max_iter", 1001), ("max_joint_step", 0.0), ("max_joint_step", -1.0), ("max_joint_step", float("nan")),
                       ("max_joint_step", float("inf")), ("tol_pos", 0.0), ("tol_pos", float("nan")), ("tol_axis", float("inf")),
                       ("nobs", -1), ("nobs", 33), ("lo", None), ("hi", None), ("obs", None), ("D", None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        refused()
        setattr(d, field, keep)
    for arr, idx, bad in ((c.lo, 0, np.nan), (c.lo, 1, 10.0), (c.hi, 2, np.inf), (c.obs, (0, 0), np.nan), (c.D, 0, np.inf)):
        keep = arr[idx]
        arr[idx] = bad
        refused()
        arr[idx] = keep
    w = np.ones(5)
    d.weight = p(w)
    for bad in (0.0, -1.0, np.nan, np.inf):
        w[3] = bad
        refused()
    d.weight = None
    for q in range(3):
        d.tool_axis[q] = 0.0
    refused()                                                             # use_axis with a zero tool axis
    d.tool_axis[2] = float("nan")
    refused()
    d.tool_axis[2] = 1.0
    d.tool[1] = float("inf")
    refused()
    d.tool[1] = 0.0
    assert call() in (0, -2)
    z[:] = 7.0
    zi[:] = 7
    refused(T=0)
    refused(s=None)
    refused(a=None)
    refused(b=None)                                                       # use_axis without target_axis
    refused(r=None)
    refused(out=None)
    refused(out=_lib.cfs_cart_out())
    refused(b=np.zeros((2, 3)))                                           # a zero target axis
    refused(a=np.full((2, 3), np.nan))
    refused(r=np.full((2, 5), np.nan))
    # the device entry: the same refusals, and `path` needs `cand_path`, its workspace
    dev = lambda out=o, T=2: lib.cfs_cart_path_device(C.byref(d), T, p(st), p(ss), p(tp), p(tp), p(tr), C.byref(out), None)  # noqa: E731
    assert dev(T=0) == -1
    o2 = _lib.cfs_cart_out()
    o2.theta, o2.status, o2.path = o.theta, o.status, p(np.zeros(2 * 17 * 5))
    assert dev(out=o2) == -1 and b"cand_path" in lib.cfs_last_error()
    assert (z == 7.0).all() and (zi == 7).all()
    # a start that is not finite is not a refusal: it is state 5 (checked on the GPU); the call is well formed
    st[0, 0, 0] = np.nan
    assert call() in (0, -2)


class _Stub(pkg.RRTCFSPlanner):
    """plan_to_pose's argument checks without a handle (they run before any GPU call)"""

    def __init__(self, meshes=()):
        import torch
        pobs, s, *_ = pkg.RRTstar_problem()
        self.K, self.max_slots, self.nj, self.device = 6, 4, 5, torch.device("cuda", 0)
        self._meshes, self._pobs, self._sys_rrt, self._ik, self._ik_limits, self._cart = list(meshes), pobs, s, {}, "robot", {}

    def plan(self, *a, **k):
        raise AssertionError("reached the device")


X0, TP, TA = np.zeros(5), np.zeros(3), np.array([0.0, 0.0, 1.0])


@pytest.mark.parametrize("kw", [
    dict(approach=0.0), dict(approach=-0.1), dict(approach=float("nan")), dict(approach=float("inf")), dict(approach="near"),
    dict(approach=True), dict(approach=[0.1] * 5), dict(approach=np.zeros((1, 1))), dict(approach=[0.1, -0.1, 0.1, 0.1]),
    dict(approach=0.1, approach_dir=[0, 0]), dict(approach=0.1, approach_dir=[0, 0, 0]), dict(approach=0.1, approach_dir=[0, np.nan, 1]),
    dict(approach=0.1, approach_dir=np.ones((5, 3))), dict(approach_dir=[0, 0, 1]),
    dict(approach=0.1, approach_steps=0), dict(approach=0.1, approach_steps=257), dict(approach=0.1, approach_steps=4.0),
    dict(approach_options=dict(max_iter=5)),
    dict(approach=0.1, approach_options=[]), dict(approach=0.1, approach_options=dict(steps=4)), dict(approach=0.1, approach_options=dict(max_iter=0)),
    dict(approach=0.1, approach_options=dict(max_joint_step=0)), dict(approach=0.1, approach_options=dict(device=0)),
])
def test_plan_to_pose_approach_arguments_are_validated_before_the_device(kw):
    with pytest.raises(ValueError):
        _Stub().plan_to_pose(X0, TP, TA, **kw)


def test_plan_to_pose_approach_needs_an_axis_and_no_meshes():
    with pytest.raises(ValueError, match="target_axis"):
        _Stub().plan_to_pose(X0, TP, None, approach=0.1)
    with pytest.raises(ValueError, match="mesh"):
        _Stub(meshes=[object()]).plan_to_pose(X0, TP, TA, approach=0.1, ik_meshes=True)
