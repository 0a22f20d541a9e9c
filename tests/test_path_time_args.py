"""Path timing: the entry points exist and are bound, and every refusal of PathTimer, of time / time_device, of the planner's
path_timing / approach_timing and of the two C entry points themselves happens before the device is touched.  No compute calls here
(CPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from test_cart_args import ROBOT, _Stub

ENTRIES = ("cfs_path_time", "cfs_path_time_device")
V, A = np.ones(5), 2 * np.ones(5)


def test_entry_points_are_exported_bound_and_documented():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(h, n) and n in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                               # purely additive
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfs_hip.h")).read()
    assert "/* ---- Path timing" in hdr and hdr.index("/* ---- Path timing") > hdr.index("int cfs_cart_follow_mesh_device(")
    for n in ENTRIES:
        assert f"int {n}(" in hdr
    assert pkg.PathTimer is pkg.timing.PathTimer and callable(pkg.PathTimer.time) and callable(pkg.PathTimer.time_device)
    # the struct layouts follow from the header's field lists
    assert C.sizeof(_lib.cfs_time_desc) == C.sizeof(_lib.cfs_robot) + 8 + 3 * 8 + 2 * 8 + 2 * 8 + 8
    assert C.sizeof(_lib.cfs_time_out) == 6 * 8


@pytest.mark.parametrize("kw", [
    dict(vmax=0.0), dict(vmax=-1.0), dict(vmax=np.ones(4)), dict(vmax=[1, 1, 1, 1, np.nan]), dict(vmax=[1, 1, 1, 1, np.inf]), dict(vmax="fast"),
    dict(vmax=np.ones((5, 1))), dict(amax=0.0), dict(amax=[2, 2, 2, 2, 0]), dict(amax=np.ones(6)), dict(amax=None),
    dict(feed=0.0), dict(feed=-0.1), dict(feed=float("nan")), dict(feed=float("inf")), dict(feed="slow"), dict(feed=True),
    dict(tool=[0, 0]), dict(tool=[0, 0, float("nan")]),
    dict(curve_share=0.0), dict(curve_share=1.0), dict(curve_share=1.5), dict(curve_share=-0.1), dict(curve_share=float("nan")), dict(curve_share="half"),
    dict(stops="all"), dict(stops=1), dict(stops=0), dict(stops=-2), dict(stops=2.0), dict(stops=True), dict(stops=None),
    dict(njoint=1), dict(njoint=7), dict(njoint=5.0), dict(device="cpu"),
])
def test_timer_arguments_are_validated(kw):
    kw = dict(dict(vmax=V, amax=A), **kw)
    with pytest.raises(ValueError):
        pkg.PathTimer(ROBOT, **kw)


def test_timer_defaults():
    t = pkg.PathTimer(ROBOT, 1.0, 2.0)
    assert t.nj == 5 and t.feed == float("inf") and t.curve_share == 0.5 and t.stops == "ends"
    assert (t.vmax == 1.0).all() and (t.amax == 2.0).all() and t.vmax.shape == (5,)
    np.testing.assert_array_equal(t.tool, pkg.ik.default_tool(ROBOT, 5)[0])
    assert pkg.PathTimer(ROBOT, V, A, stops=4)._stop_every(None) == 4 and pkg.PathTimer(ROBOT, V, A, stops="corners")._stop_every(3) == 3
    assert pkg.PathTimer(pkg.robotproperty2("2L"), 1.0, 1.0).nj == 2


P17 = np.zeros((2, 3, 17, 5))


@pytest.mark.parametrize("args,kw,tkw", [
    ((np.zeros(5),), {}, {}), ((np.zeros((17, 4)),), {}, {}), ((np.zeros((2, 2, 5)),), {}, {}), ((np.zeros((258, 5)),), {}, {}),
    ((np.zeros((0, 17, 5)),), {}, {}), ((np.zeros((2, 0, 17, 5)),), {}, {}), ((np.zeros((2, 65, 17, 5)),), {}, {}), ((np.zeros((1, 2, 3, 17, 5)),), {}, {}),
    (("along",), {}, {}), ((None,), {}, {}),
    ((P17,), dict(state=np.zeros((2, 4), np.int32)), {}), ((P17,), dict(state=np.zeros((2, 3))), {}), ((P17,), dict(state="all"), {}),
    ((P17[0],), dict(state=np.zeros((3, 1), np.int32)), {}), ((P17[0, 0],), dict(state=np.zeros(1, np.int32)), {}),
    ((P17,), {}, dict(stops="corners")), ((P17,), dict(steps=1), dict(stops="corners")), ((P17,), dict(steps=4.0), dict(stops="corners")),
    ((P17,), dict(steps=0), {}), ((P17,), dict(steps=True), {}),
])
def test_time_arguments_are_validated_before_the_library(args, kw, tkw, monkeypatch):
    t = pkg.PathTimer(ROBOT, V, A, **tkw)
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    with pytest.raises(ValueError):
        t.time(*args, **kw)
    with pytest.raises(ValueError):
        t.time_device(*args, **kw)                                        # host arrays are not CUDA tensors either


def test_time_shapes_and_the_call(monkeypatch):
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    t = pkg.PathTimer(ROBOT, V, A, feed=0.25, stops="corners", curve_share=0.25)
    r = t.time(P17, state=np.zeros((2, 3), np.int64), steps=4)
    assert r.time.shape == r.sdot.shape == (2, 3, 17) and r.duration.shape == r.status.shape == (2, 3)
    assert r.selected.shape == r.group_status.shape == (2,) and r.status.dtype == np.int32 and r.selected.dtype == np.int32
    r = t.time(P17[0], steps=4)                                           # (T, N, nj): T groups of one path
    assert r.time.shape == (3, 17) and r.duration.shape == (3,) and r.selected.shape == (3,)
    r = pkg.PathTimer(ROBOT, V, A).time(P17[0, 0], state=0)              # one path
    assert r.time.shape == (17,) and r.duration.shape == () and r.selected.shape == ()
    assert [n for n, _ in calls] == ["cfs_path_time"] * 3
    a = calls[0][1]
    assert len(a) == 7 and a[1:4] == (2, 3, 17) and a[5] is not None
    d = a[0]._obj
    assert d.njoint == 5 and d.feed == 0.25 and d.curve_share == 0.25 and d.stop_every == 4
    assert calls[1][1][1:4] == (3, 1, 17) and calls[1][1][5] is None
    d = calls[2][1][0]._obj
    assert calls[2][1][1:4] == (1, 1, 17) and d.feed == float("inf") and d.stop_every == 0


def test_c_entry_points_refuse_bad_arguments_and_write_nothing():
    lib = pkg.lib()
    t = pkg.PathTimer(ROBOT, V.copy(), A.copy(), feed=0.2)
    d = t._desc(None)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    G, R, N = 2, 3, 9
    paths, state = np.zeros((G, R, N, 5)), np.zeros((G, R), np.int32)
    z, zi = np.full(G * R * N * 2 + G * R, 7.0), np.full(G * R + 2 * G, 7, np.int32)

    def outs(time=True, sdot=True, duration=True, status=True, groups=True):
        o = _lib.cfs_time_out()
        if time:
            o.time = p(z[:G * R * N])
        if sdot:
            o.sdot = p(z[G * R * N:2 * G * R * N])
        if duration:
            o.duration = p(z[2 * G * R * N:])
        if status:
            o.status = p(zi[:G * R])
        if groups:
            o.selected, o.group_status = p(zi[G * R:G * R + G]), p(zi[G * R + G:])
        return o

    def call(entry, G_=G, R_=R, N_=N, a=paths, s=state, out="all", d_=d):
        out = outs() if isinstance(out, str) else out
        return getattr(lib, entry)(C.byref(d_) if d_ is not None else None, G_, R_, N_, p(a), p(s), C.byref(out) if out is not None else None,
                                   *((None,) if entry.endswith("_device") else ()))

    def refused(only=ENTRIES, **kw):
        for e in only:
            assert call(e, **kw) == -1 and lib.cfs_last_error(), (e, kw)
            assert (z == 7.0).all() and (zi == 7).all()                   # nothing written
    if pkg.device_count() == 0:
        for e in ENTRIES:                                                # well formed: no device (never a crash, never a CPU fallback)
            assert call(e) == -2 and b"device" in lib.cfs_last_error().lower(), e
            assert call(e, s=None, out=outs(time=False, groups=False)) == -2
        assert call("cfs_path_time", out=outs(time=False, sdot=False)) == -2     # the host entry stages its own workspace
        assert (z == 7.0).all() and (zi == 7).all()
    assert call("cfs_path_time_device", out=outs(time=False, sdot=False)) == -1 and b"cfs_path_time_device" in lib.cfs_last_error()
    # the batch
    for bad in (0, -1):
        refused(G_=bad)
    for bad in (0, -1, 65):
        refused(R_=bad)
    for bad in (2, 0, -4, 258):
        refused(N_=bad)
    refused(G_=2 ** 30, R_=64)                                           # more paths than an int counts
    # the descriptor
    refused(d_=None)
    for field, bad in (("njoint", 1), ("njoint", 7), ("njoint", 0), ("stop_every", 1), ("stop_every", -1), ("stop_every", -8),
                       ("feed", 0.0), ("feed", -1.0), ("feed", float("nan")), ("feed", float("-inf")),
                       ("curve_share", 0.0), ("curve_share", 1.0), ("curve_share", -0.5), ("curve_share", float("nan")), ("curve_share", float("inf")),
                       ("vmax", None), ("amax", None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        refused()
        setattr(d, field, keep)
    keep = d.robot.kind
    d.robot.kind = 9
    refused()
    d.robot.kind = keep
    keep = d.robot.nlink
    d.robot.nlink = 0
    refused()
    d.robot.nlink = keep
    for arr in (t.vmax, t.amax):
        for bad in (0.0, -1.0, np.nan, np.inf):
            keep = arr[3]
            arr[3] = bad
            refused()
            arr[3] = keep
    keep = d.tool[1]
    d.tool[1] = float("nan")
    refused()                                                             # a finite feed reads the tool point
    d.feed = float("inf")
    if pkg.device_count() == 0:
        assert call("cfs_path_time") == -2                                # without a feed it is not read
    d.feed, d.tool[1] = 0.2, keep
    d.stop_every = 2
    if pkg.device_count() == 0:
        assert call("cfs_path_time") == -2 and call("cfs_path_time_device") == -2
    d.stop_every = 0
    # the arrays
    refused(a=None)
    refused(out=None)
    refused(out=_lib.cfs_time_out())
    refused(out=outs(duration=False))
    refused(out=outs(status=False))
    refused(out=outs(sdot=False))                                         # time without sdot
    assert b"sdot" in lib.cfs_last_error()
    # a row that is not finite is not a refusal: it is status 2 (checked on the GPU); the call is well formed
    paths[0, 0, 0, 0] = np.nan
    assert call("cfs_path_time") in (0, -2)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
X0 = np.zeros(5)
P3 = np.zeros((3, 3))
A3 = np.tile([0.0, 0.0, 1.0], (3, 1))
TIMING = dict(vmax=1.0, amax=2.0)


@pytest.mark.parametrize("kw", [
    dict(path_timing=[]), dict(path_timing="fast"), dict(path_timing={}), dict(path_timing=dict(vmax=1.0)), dict(path_timing=dict(amax=1.0)),
    dict(path_timing=dict(TIMING, tool=[0, 0, 0])), dict(path_timing=dict(TIMING, steps=4)), dict(path_timing=dict(TIMING, device=0)),
    dict(path_timing=dict(vmax=0.0, amax=2.0)), dict(path_timing=dict(vmax=1.0, amax=np.ones(4))), dict(path_timing=dict(TIMING, feed=0.0)),
    dict(path_timing=dict(TIMING, feed=float("inf"))), dict(path_timing=dict(TIMING, stops="all")), dict(path_timing=dict(TIMING, stops=1)),
    dict(path_timing=dict(TIMING, curve_share=1.0)),
    dict(path_timing=dict(TIMING, stops="corners"), path_steps=1),                                              # one sub-step: every row rests
    dict(path_timing=TIMING, path_steps=1, path_pos=np.zeros((2, 3)), path_axis=np.tile([0.0, 0.0, 1.0], (2, 1))),   # a path of two rows
])
def test_plan_to_path_timing_is_validated_before_the_device(kw):
    kw = dict(kw)
    args = [kw.pop("x0", X0), kw.pop("path_pos", P3), kw.pop("path_axis", A3)]
    with pytest.raises(ValueError):
        _Stub().plan_to_path(*args, **kw)


@pytest.mark.parametrize("kw", [
    dict(approach_timing=TIMING), dict(approach=0.05, approach_timing=[]), dict(approach=0.05, approach_timing=dict(vmax=1.0)),
    dict(approach=0.05, approach_timing=dict(TIMING, feed=-1.0)), dict(approach=0.05, approach_timing=dict(TIMING, max_iter=3)),
    dict(approach=0.05, approach_timing=TIMING, approach_steps=1),                                               # a path of two rows
    dict(approach=0.05, approach_timing=dict(TIMING, stops="corners"), approach_steps=1),
])
def test_plan_to_pose_timing_is_validated_before_the_device(kw):
    with pytest.raises(ValueError):
        _Stub().plan_to_pose(X0, np.zeros(3), np.array([0.0, 0.0, 1.0]), **kw)
