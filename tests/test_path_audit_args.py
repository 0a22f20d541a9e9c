"""Tool-path audit: the entry points exist and are bound, and every refusal of PathAudit, of audit / audit_device, of the planner's
path_audit / approach_audit and of the two C entry points themselves happens before the device is touched.  No compute calls here
(CPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from test_cart_args import LINE, ROBOT, _Stub

ENTRIES = ("cfs_path_audit", "cfs_path_audit_device")
INF = float("inf")


def test_entry_points_are_exported_bound_and_documented():
    h = C.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(h, n) and n in [s[0] for s in _lib.SYMBOLS]
    assert pkg.lib().cfs_abi_version() == 1                               # purely additive
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfs_hip.h")).read()
    assert "/* ---- Tool-path audit" in hdr and hdr.index("/* ---- Tool-path audit") > hdr.index("int cfs_path_time_device(")
    for n in ENTRIES:
        assert f"int {n}(" in hdr
    assert pkg.PathAudit is pkg.audit.PathAudit and callable(pkg.PathAudit.audit) and callable(pkg.PathAudit.audit_device)
    # the struct layouts follow from the header's field lists
    assert C.sizeof(_lib.cfs_audit_desc) == C.sizeof(_lib.cfs_robot) + 8 + 3 * 8 + 8 + 2 * 8 + 8 + 2 * 8
    assert C.sizeof(_lib.cfs_audit_out) == 10 * 8
    assert _lib.PATH_AUDIT_STATE[6] and _lib.PATH_AUDIT_STATE[7] and all(_lib.PATH_AUDIT_STATE[k] == v for k, v in _lib.CART_CAND_STATUS.items())


class _FakeMesh:
    pass


@pytest.mark.parametrize("kw", [
    dict(tool=[0, 0]), dict(tool=[0, 0, float("nan")]), dict(tool="tip"),
    dict(min_clearance=float("nan")), dict(min_clearance=INF), dict(min_clearance=-INF), dict(min_clearance="wide"), dict(min_clearance=True),
    dict(max_chord=0.0), dict(max_chord=-1e-3), dict(max_chord=float("nan")), dict(max_chord=INF), dict(max_chord="small"),
    dict(njoint=1), dict(njoint=7), dict(njoint=5.0), dict(device="cpu"),
    dict(obs=[dict(l=np.zeros((2, 3)), D=0.1)]), dict(obs=[dict(l=np.full((3, 2), np.nan), D=0.1)]), dict(obs=[dict(l=np.zeros((3, 2)))]),
    dict(obs=[dict(l=np.zeros((3, 2)), D=float("nan"))]), dict(obs=[LINE] * 33), dict(obs=7), dict(obs=["line"]),
])
def test_audit_construction_is_validated(kw):
    kw = dict(kw)
    obs = kw.pop("obs", [LINE])
    with pytest.raises(ValueError):
        pkg.PathAudit(ROBOT, obs, **kw)


def test_meshes_are_refused_in_words():
    for cell in ([LINE, dict(mesh=_FakeMesh(), D=0.05)], [dict(mesh=_FakeMesh(), D=0.05, pose=np.eye(4))], [dict(LINE, pose=np.eye(4))]):
        with pytest.raises(ValueError, match="meshes are not audited"):
            pkg.PathAudit(ROBOT, cell)


def test_audit_defaults():
    a = pkg.PathAudit(ROBOT, None)
    assert a.nj == 5 and a.min_clearance == -INF and a.max_chord == INF and a.obs.shape == (0, 6) and a.D.shape == (0,)
    np.testing.assert_array_equal(a.tool, pkg.ik.default_tool(ROBOT, 5)[0])
    a = pkg.PathAudit(ROBOT, [LINE, LINE], min_clearance=-0.01, max_chord=1e-3)
    assert a.obs.shape == (2, 6) and a.min_clearance == -0.01 and a.max_chord == 1e-3
    assert pkg.PathAudit(pkg.robotproperty2("2L"), []).nj == 2


P17 = np.zeros((2, 3, 17, 5))


@pytest.mark.parametrize("args,kw", [
    ((np.zeros(5),), {}), ((np.zeros((17, 4)),), {}), ((np.zeros((2, 2, 6)),), {}), ((np.zeros((258, 5)),), {}), ((np.zeros((1, 5)),), {}),
    ((np.zeros((0, 17, 5)),), {}), ((np.zeros((2, 0, 17, 5)),), {}), ((np.zeros((2, 65, 17, 5)),), {}), ((np.zeros((1, 2, 3, 17, 5)),), {}),
    (("along",), {}), ((None,), {}),
    ((P17,), dict(state=np.zeros((2, 4), np.int32))), ((P17,), dict(state=np.zeros((2, 3)))), ((P17,), dict(state="all")),
    ((P17[0],), dict(state=np.zeros((3, 1), np.int32))), ((P17[0, 0],), dict(state=np.zeros(1, np.int32))),
    ((P17,), dict(substeps=0)), ((P17,), dict(substeps=65)), ((P17,), dict(substeps=4.0)), ((P17,), dict(substeps=True)), ((P17,), dict(substeps=None)),
])
def test_audit_arguments_are_validated_before_the_library(args, kw, monkeypatch):
    a = pkg.PathAudit(ROBOT, [LINE])
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    with pytest.raises(ValueError):
        a.audit(*args, **kw)
    with pytest.raises(ValueError):
        a.audit_device(*args, **kw)                                       # host arrays are not CUDA tensors either


def test_audit_shapes_and_the_call(monkeypatch):
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    a = pkg.PathAudit(ROBOT, [LINE], min_clearance=0.0, max_chord=2e-3)
    r = a.audit(P17, state=np.zeros((2, 3), np.int64), substeps=5)
    for k in ("clear_rows", "clear_path", "s_path", "clear_lower", "chord_err", "chord_upper", "link_path", "obs_path", "status", "state_out"):
        assert getattr(r, k).shape == (2, 3), k
    assert r.status.dtype == r.state_out.dtype == r.link_path.dtype == np.int32 and r.clear_lower.dtype == np.float64
    r = a.audit(P17[0])                                                   # (T, N, nj): T groups of one path
    assert r.clear_path.shape == (3,)
    r = pkg.PathAudit(ROBOT, None).audit(np.zeros((2, 5)), state=0, substeps=64)   # one path of two rows, no obstacles
    assert r.clear_path.shape == () and r.status.shape == ()
    assert [n for n, _ in calls] == ["cfs_path_audit"] * 3
    c = calls[0][1]
    assert len(c) == 7 and c[1:4] == (2, 3, 17) and c[5] is not None
    d = c[0]._obj
    assert (d.njoint, d.nobs, d.substeps, d.min_clearance, d.max_chord) == (5, 1, 5, 0.0, 2e-3) and d.obs and d.D
    assert calls[1][1][1:4] == (3, 1, 17) and calls[1][1][5] is None and calls[1][1][0]._obj.substeps == 8
    d = calls[2][1][0]._obj
    assert calls[2][1][1:4] == (1, 1, 2) and (d.nobs, d.substeps, d.min_clearance, d.max_chord) == (0, 64, -INF, INF) and not d.obs and not d.D


def test_c_entry_points_refuse_bad_arguments_and_write_nothing():
    lib = pkg.lib()
    a = pkg.PathAudit(ROBOT, [LINE, LINE], min_clearance=0.0, max_chord=1e-3)
    obs, D = a.obs.copy(), a.D.copy()
    d = a._desc(4, obs, D)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    G, R, N = 2, 3, 9
    paths, state = np.zeros((G, R, N, 5)), np.zeros((G, R), np.int32)
    z, zi = np.full(6 * G * R, 7.0), np.full(4 * G * R, 7, np.int32)
    names = [k for k, _ in _lib.cfs_audit_out._fields_]

    def outs(skip=()):
        o = _lib.cfs_audit_out()
        f = i = 0
        for k in names:
            if k in ("link_path", "obs_path", "status", "state_out"):
                v, i = p(zi[i * G * R:(i + 1) * G * R]), i + 1
            else:
                v, f = p(z[f * G * R:(f + 1) * G * R]), f + 1
            if k not in skip:
                setattr(o, k, v)
        return o

    def call(entry, G_=G, R_=R, N_=N, a_=paths, s=state, out="all", d_=d):
        out = outs() if isinstance(out, str) else out
        return getattr(lib, entry)(C.byref(d_) if d_ is not None else None, G_, R_, N_, p(a_), p(s), C.byref(out) if out is not None else None,
                                   *((None,) if entry.endswith("_device") else ()))

    def refused(only=ENTRIES, **kw):
        for e in only:
            assert call(e, **kw) == -1 and lib.cfs_last_error(), (e, kw)
            assert (z == 7.0).all() and (zi == 7).all()                   # nothing written
    if pkg.device_count() == 0:
        for e in ENTRIES:                                                # well formed: no device (never a crash, never a CPU fallback)
            assert call(e) == -2 and b"device" in lib.cfs_last_error().lower(), e
            assert call(e, s=None, out=outs(skip=[k for k in names if k != "status"])) == -2
            assert call(e, N_=2) == -2 and call(e, R_=64, G_=1) == -2
        assert (z == 7.0).all() and (zi == 7).all()
    # the batch
    for bad in (0, -1):
        refused(G_=bad)
    for bad in (0, -1, 65):
        refused(R_=bad)
    for bad in (1, 0, -4, 258):
        refused(N_=bad)
    refused(G_=2 ** 30, R_=64)                                           # more paths than an int counts
    # the descriptor
    refused(d_=None)
    nan = float("nan")
    for field, bad in (("njoint", 1), ("njoint", 7), ("njoint", 0), ("substeps", 0), ("substeps", -1), ("substeps", 65), ("nobs", -1), ("nobs", 33),
                       ("min_clearance", nan), ("min_clearance", INF), ("max_chord", nan), ("max_chord", 0.0), ("max_chord", -1.0), ("max_chord", -INF),
                       ("obs", None), ("D", None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        refused()
        setattr(d, field, keep)
    for field, bad in (("kind", 9), ("nlink", 0)):
        keep = getattr(d.robot, field)
        setattr(d.robot, field, bad)
        refused()
        setattr(d.robot, field, keep)
    for bad in (nan, INF):
        keep = d.tool[1]
        d.tool[1] = bad
        refused()
        d.tool[1] = keep
    # the arrays
    refused(a_=None)
    refused(out=None)
    refused(out=_lib.cfs_audit_out())
    refused(out=outs(skip=["status"]))
    # values the host can read: the host entry refuses them, the device entry cannot
    for arr in (obs, D):
        for bad in (nan, INF):
            keep = arr.flat[1]
            arr.flat[1] = bad
            refused(only=ENTRIES[:1])
            if pkg.device_count() == 0:
                assert call(ENTRIES[1]) == -2
            arr.flat[1] = keep
    # both thresholds off, no obstacles and no pointers to them: well formed
    d.nobs, d.min_clearance, d.max_chord = 0, -INF, INF
    keep = d.obs, d.D
    d.obs = d.D = None
    if pkg.device_count() == 0:
        assert call(ENTRIES[0]) == -2 and call(ENTRIES[1]) == -2
    d.obs, d.D = keep
    d.nobs, d.min_clearance, d.max_chord = 2, 0.0, 1e-3
    # a row that is not finite is not a refusal: it is status 2 (checked on the GPU); the call is well formed
    paths[0, 0, 0, 0] = np.nan
    assert call("cfs_path_audit") in (0, -2)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
X0 = np.zeros(5)
P3 = np.zeros((3, 3))
A3 = np.tile([0.0, 0.0, 1.0], (3, 1))


@pytest.mark.parametrize("kw", [
    dict(path_audit=[]), dict(path_audit="strict"), dict(path_audit=True), dict(path_audit=dict(steps=4)), dict(path_audit=dict(tool=[0, 0, 0])),
    dict(path_audit=dict(device=0)), dict(path_audit=dict(substeps=0)), dict(path_audit=dict(substeps=65)), dict(path_audit=dict(substeps=2.0)),
    dict(path_audit=dict(min_clearance=float("nan"))), dict(path_audit=dict(min_clearance=INF)), dict(path_audit=dict(max_chord=0.0)),
    dict(path_audit=dict(max_chord=-1.0)), dict(path_audit=dict(max_chord="small")),
])
def test_plan_to_path_audit_is_validated_before_the_device(kw):
    with pytest.raises(ValueError):
        _Stub().plan_to_path(X0, P3, A3, **kw)


@pytest.mark.parametrize("kw", [
    dict(approach_audit={}), dict(approach=0.05, approach_audit=[]), dict(approach=0.05, approach_audit=dict(substeps=0)),
    dict(approach=0.05, approach_audit=dict(max_chord=0.0)), dict(approach=0.05, approach_audit=dict(max_iter=3)),
    dict(approach=0.05, approach_audit=dict(min_clearance="wide")),
])
def test_plan_to_pose_audit_is_validated_before_the_device(kw):
    with pytest.raises(ValueError):
        _Stub().plan_to_pose(X0, np.zeros(3), np.array([0.0, 0.0, 1.0]), **kw)


def test_a_planner_with_meshes_refuses_the_audit():
    with pytest.raises(ValueError, match="meshes are not audited"):
        _Stub(meshes=[object()]).plan_to_path(X0, P3, A3, ik_meshes=True, path_meshes=True, path_audit={})
    with pytest.raises(ValueError, match="meshes are not audited"):
        _Stub(meshes=[object()]).plan_to_pose(X0, np.zeros(3), np.array([0.0, 0.0, 1.0]), ik_meshes=True, approach=0.05, approach_meshes=True,
                                             approach_audit={})
