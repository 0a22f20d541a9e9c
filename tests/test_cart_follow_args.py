"""Tool paths: the entry points exist and are bound, and every refusal of CartesianPath.follow / follow_device, of plan_to_path and of
the four C entry points themselves happens before the device is touched.  No compute calls here (CPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from test_cart_args import LINE, ROBOT, _Stub, _desc
from test_ik_mesh_args import _mesh

ENTRIES = ("cfs_cart_follow", "cfs_cart_follow_device", "cfs_cart_follow_mesh", "cfs_cart_follow_mesh_device")


def test_entry_points_are_exported_bound_and_documented():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(h, n) and n in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                               # purely additive
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfs_hip.h")).read()
    assert "/* ---- Tool paths" in hdr and hdr.index("/* ---- Tool paths") > hdr.index("int cfs_cart_path_mesh_device(")
    for n in ENTRIES:
        assert f"int {n}(" in hdr
    assert callable(pkg.CartesianPath.follow) and callable(pkg.CartesianPath.follow_device) and callable(pkg.RRTCFSPlanner.plan_to_path)


S1 = np.zeros((1, 4, 5))
P3 = np.zeros((3, 3))
A3 = np.tile([0.0, 0.0, 1.0], (3, 1))


@pytest.mark.parametrize("args,kw", [
    ((np.zeros(5), P3), {}), ((np.zeros((1, 4, 4)), P3), {}), ((np.zeros((1, 65, 5)), P3), {}), ((np.zeros((1, 0, 5)), P3), {}), (("here", P3), {}),
    ((S1, np.zeros(3)), {}), ((S1, np.zeros((1, 3))), {}), ((S1, np.zeros((258, 3))), {}), ((S1, np.zeros((3, 2))), {}), ((S1, "along"), {}),
    ((S1, np.zeros((0, 3, 3))), {}), ((S1, np.zeros((1, 1, 3, 3))), {}), ((S1, np.zeros((18, 3))), {}),          # 17 segments x 16 steps > 256
    ((S1, np.full((3, 3), np.nan)), {}), ((S1, np.array([[0, 0, 0], [0, np.inf, 0], [0, 0, 0.0]])), {}),
    ((np.zeros((2, 4, 5)), np.zeros((3, 3, 3))), {}),                                                            # start and path_pos disagree on T
    ((S1, P3, np.zeros((3, 3))), {}), ((S1, P3, np.zeros((2, 3))), {}), ((S1, P3, np.array([[0, 0, 1], [0, np.nan, 1], [0, 0, 1.0]])), {}),
    ((S1, P3, np.zeros((1, 3, 3, 1))), {}), ((S1, P3, [0, 0, 1]), {}), ((S1, P3, "up"), {}),
    ((S1, P3, None, np.zeros(4)), {}), ((S1, P3, None, np.full(5, np.inf)), {}),
    ((S1, P3), dict(start_state=np.zeros((1, 3), np.int32))), ((S1, P3), dict(start_state=np.zeros((1, 4)))), ((S1, P3), dict(start_state="all")),
])
def test_follow_arguments_are_validated_before_the_library(args, kw, monkeypatch):
    c = pkg.CartesianPath(ROBOT, [LINE])
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    with pytest.raises(ValueError):
        c.follow(*args, **kw)
    with pytest.raises(ValueError):
        c.follow_device(*args, **kw)                                      # host arrays are not CUDA tensors either


def test_the_row_limit_follows_the_solvers_steps(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    with pytest.raises(ValueError, match="at most 256 rows"):
        pkg.CartesianPath(ROBOT, steps=128).follow(S1, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="2..257 poses"):
        pkg.CartesianPath(ROBOT, steps=1).follow(S1, np.zeros((258, 3)))
    with pytest.raises(AssertionError, match="reached the library"):      # 256 segments of one step, and 2 of 128, are well formed
        pkg.CartesianPath(ROBOT, steps=1).follow(S1, np.zeros((257, 3)))
    with pytest.raises(AssertionError, match="reached the library"):
        pkg.CartesianPath(ROBOT, steps=128).follow(S1, np.zeros((3, 3)))


def test_follow_routes_to_the_four_entries(monkeypatch):
    """the host entries get npts behind T (and the mesh table between the descriptor and T); trace keeps its entries"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    start, pos = np.zeros((2, 3, 5)), np.ones((2, 4, 3))
    axs = np.tile([0.0, 0.0, 1.0], (2, 4, 1))
    line = pkg.CartesianPath(ROBOT, [LINE], steps=5)
    r = line.follow(start, pos, axs, want_candidates=True)
    assert r.path.shape == (2, 16, 5) and r.cand_path.shape == (2, 3, 16, 5) and r.theta.shape == (2, 5)
    one = line.follow(start[0], pos[0])                                   # (R, nj) and (M, 3): one target, position only
    assert one.path.shape == (1, 16, 5) and not hasattr(one, "cand_path")
    pkg.CartesianPath(ROBOT, [LINE, dict(mesh=_mesh(), D=0.25)], meshes=True, mesh_variant="per_lane", steps=5).follow(start, pos, axs)
    line.trace(start, np.ones((2, 3)))
    assert [n for n, _ in calls] == ["cfs_cart_follow", "cfs_cart_follow", "cfs_cart_follow_mesh", "cfs_cart_path"]
    a = calls[0][1]
    assert len(a) == 9 and a[1] == 2 and a[2] == 4 and a[6] is not None                      # T, npts, path_axis
    assert calls[1][1][1] == 1 and calls[1][1][2] == 4 and calls[1][1][6] is None           # no axis: position only
    m = calls[2][1]
    assert len(m) == 13 and m[1] == 1 and m[4] == 1 and m[5] == 2 and m[6] == 4              # nmesh, flags, T, npts
    assert a[0]._obj.steps == 5 and a[0]._obj.use_axis == 1 and calls[1][1][0]._obj.use_axis == 0   # steps stays the sub-steps per segment


def test_c_entry_points_refuse_bad_arguments_and_write_nothing():
    lib = pkg.lib()
    c, d, o, z, zi = _desc()
    d.steps = 4
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    M = 3
    st, ss, tr = np.zeros((2, 4, 5)), np.zeros((2, 4), np.int32), np.zeros((2, 5))
    pos, axs = np.ones((2, M, 3)), np.tile([0.0, 0.0, 1.0], (2, M, 1))
    work = np.zeros(2 * 4 * 9 * 5)
    o.cand_path = p(work)                                                # the device entries' workspace
    fake = np.zeros(64, np.int64)                                        # an empty mesh of device 0: no triangles, nothing to read
    arr = (C.c_void_p * 2)(fake.ctypes.data, fake.ctypes.data)
    Dm = np.array([0.1, 0.2])
    q = lambda x: None if x is None else p(x)  # noqa: E731

    def call(entry, T=2, npts=M, s=st, a=pos, b=axs, r=tr, out=o, nmesh=2, meshes=arr, D=Dm, flags=0, d_=d):
        tail = (T, npts, q(s), p(ss), q(a), q(b), q(r), C.byref(out) if out is not None else None)
        head = (C.byref(d_) if d_ is not None else None,) + ((nmesh, meshes, q(D), flags) if "mesh" in entry else ())
        return getattr(lib, entry)(*head, *tail, *((None,) if entry.endswith("_device") else ()))
    if pkg.device_count() == 0:
        for e in ENTRIES:                                                # well formed: no device (never a crash, never a CPU fallback)
            assert call(e) == -2 and b"device" in lib.cfs_last_error().lower(), e
    z[:] = 7.0
    zi[:] = 7
    work[:] = 7.0

    def refused(only=ENTRIES, **kw):
        for e in only:
            assert call(e, **kw) == -1 and lib.cfs_last_error(), (e, kw)
            assert (z == 7.0).all() and (zi == 7).all() and (work == 7.0).all()      # nothing written
    # the path table
    for bad in (1, 0, -3, 258):
        refused(npts=bad)
    refused(a=None)
    refused(b=None)                                                       # use_axis without path_axis
    assert b"path_axis" in lib.cfs_last_error()
    d.steps = 129
    refused()                                                             # 2 segments x 129 steps > 256
    assert b"(npts-1)*steps" in lib.cfs_last_error()
    d.steps = 256
    refused()
    if pkg.device_count() == 0:
        assert call("cfs_cart_follow", npts=2, a=np.ones((2, 2, 3)), b=np.tile([0.0, 0.0, 1.0], (2, 2, 1)), out=_small(o)) == -2   # 1 x 256: well formed
    d.steps = 4
    # everything cfs_cart_path* refuse about the shared fields
    refused(d_=None)
    for field, bad in (("njoint", 1), ("njoint", 7), ("use_axis", 2), ("candidates", 0), ("candidates", 65), ("steps", 0), ("steps", 257),
                       ("max_iter", 0), ("max_iter", 1001), ("max_joint_step", 0.0), ("max_joint_step", -1.0), ("max_joint_step", float("nan")),
                       ("max_joint_step", float("inf")), ("tol_pos", 0.0), ("tol_pos", float("nan")), ("tol_axis", float("inf")),
                       ("nobs", -1), ("nobs", 33), ("lo", None), ("hi", None), ("obs", None), ("D", None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        refused()
        setattr(d, field, keep)
    for arr_, idx, bad in ((c.lo, 0, np.nan), (c.lo, 1, 10.0), (c.hi, 2, np.inf)):
        keep = arr_[idx]
        arr_[idx] = bad
        refused()
        arr_[idx] = keep
    w = np.ones(5)
    d.weight = p(w)
    for bad in (0.0, -1.0, np.nan, np.inf):
        w[3] = bad
        refused()
    d.weight = None
    keep = [d.tool_axis[k] for k in range(3)]
    for k in range(3):
        d.tool_axis[k] = 0.0
    refused()                                                             # use_axis with a zero tool axis
    for k in range(3):
        d.tool_axis[k] = keep[k]
    refused(T=0)
    refused(s=None)
    refused(r=None)
    refused(out=None)
    refused(out=_lib.cfs_cart_out())
    # the mesh table, as cfs_cart_path_mesh* refuse it
    mesh = ENTRIES[2:]
    refused(mesh, nmesh=0)
    refused(mesh, meshes=None)
    refused(mesh, meshes=(C.c_void_p * 2)(fake.ctypes.data, None))
    refused(mesh, D=None)
    refused(mesh, D=np.array([0.1, np.nan]))
    for flags in (8, 1 | 2, 1 | 4):
        refused(mesh, flags=flags)
    # what only the host entries can read: a non-finite path_pos / path_axis / theta_ref / obs, a zero path_axis row
    host = ("cfs_cart_follow", "cfs_cart_follow_mesh")
    bad_pos, bad_axs, zero = pos.copy(), axs.copy(), axs.copy()
    bad_pos[1, 2, 0], bad_axs[1, 1, 2], zero[1, 2] = np.nan, np.inf, 0.0
    refused(host, a=bad_pos)
    refused(host, b=bad_axs)
    refused(host, b=zero)
    assert b"path_axis row 5 is zero" in lib.cfs_last_error()
    refused(host, r=np.full((2, 5), np.nan))
    keep = c.obs[0, 0]
    c.obs[0, 0] = np.nan
    refused(host)
    c.obs[0, 0] = keep
    # the device entries: `path` needs `cand_path` (line-only), and the mesh entry needs `cand_path` always
    o2 = _lib.cfs_cart_out()
    o2.theta, o2.status = o.theta, o.status
    assert call("cfs_cart_follow_mesh_device", out=o2) == -1 and b"cfs_cart_follow_mesh_device" in lib.cfs_last_error()
    o2.path = p(np.zeros(2 * 9 * 5))
    assert call("cfs_cart_follow_device", out=o2) == -1 and b"cand_path" in lib.cfs_last_error() and b"cfs_cart_follow_device" in lib.cfs_last_error()
    assert call("cfs_cart_follow_mesh_device", out=o2) == -1 and b"cand_path" in lib.cfs_last_error()
    assert (z == 7.0).all() and (zi == 7).all()
    if pkg.device_count() == 0:
        assert call("cfs_cart_follow", out=o2) == -2 and call("cfs_cart_follow_mesh", out=o2) == -2   # the host entries stage the workspace
    # a start that is not finite is not a refusal: it is state 5 (checked on the GPU); the call is well formed
    st[0, 0, 0] = np.nan
    assert call("cfs_cart_follow") in (0, -2)


def _small(o):
    """`o` without the optional arrays, whose sizes belong to another shape"""
    s = _lib.cfs_cart_out()
    s.theta, s.status = o.theta, o.status
    return s


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
X0 = np.zeros(5)


@pytest.mark.parametrize("kw", [
    dict(path_steps=0), dict(path_steps=257), dict(path_steps=4.0),
    dict(path_steps=128, path_pos=np.zeros((4, 3)), path_axis=np.tile([0.0, 0.0, 1.0], (4, 1))),                # 3 segments x 128 steps > 256
    dict(path_options=[]), dict(path_options=dict(steps=4)), dict(path_options=dict(max_iter=0)), dict(path_options=dict(max_joint_step=0)),
    dict(path_options=dict(device=0)), dict(ik_options=dict(steps=3)), dict(ik_options=[]), dict(ik_meshes=1), dict(path_meshes="yes"),
    dict(path_meshes=None), dict(seed=-1), dict(seed=1.5),
    dict(path_pos=np.zeros(3)), dict(path_pos=np.zeros((1, 3))), dict(path_pos=np.zeros((258, 3))), dict(path_pos=np.zeros((2, 3, 2))),
    dict(path_pos=np.full((3, 3), np.nan)), dict(path_pos="along"), dict(path_pos=np.zeros((5, 3, 3))),        # S = 5 > max_slots = 4
    dict(path_axis=None), dict(path_axis=np.zeros((3, 3))), dict(path_axis=np.tile([0.0, 0.0, 1.0], (2, 1))),
    dict(path_axis=np.tile([0.0, np.inf, 1.0], (3, 1))), dict(x0=np.zeros(4)), dict(x0=np.zeros((2, 5)), path_pos=np.zeros((3, 3, 3)),
                                                                                    path_axis=np.tile([0.0, 0.0, 1.0], (3, 3, 1))),
])
def test_plan_to_path_arguments_are_validated_before_the_device(kw):
    kw = dict(kw)
    args = [kw.pop("x0", X0), kw.pop("path_pos", P3), kw.pop("path_axis", A3)]
    with pytest.raises(ValueError):
        _Stub().plan_to_path(*args, **kw)


def test_plan_to_path_mesh_planner_refusals():
    mesh_planner = _Stub(meshes=[object()])
    with pytest.raises(ValueError, match="ik_meshes=True"):
        mesh_planner.plan_to_path(X0, P3, A3)
    with pytest.raises(ValueError, match="ik_meshes=True"):
        mesh_planner.plan_to_path(X0, P3, A3, path_meshes=True)
    with pytest.raises(ValueError, match="path_meshes=True"):
        mesh_planner.plan_to_path(X0, P3, A3, ik_meshes=True)
    with pytest.raises(ValueError, match="path_meshes=True"):
        mesh_planner.plan_to_path(X0, P3, A3, ik_meshes=True, path_meshes=False)
