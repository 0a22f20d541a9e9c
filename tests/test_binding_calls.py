"""The wiring of the host-pointer entries: which library symbol each one calls, with which scalars, and that every pointer it
passes is the address of the argument or result field of the same name.  The library is a recorder that returns 0; shapes are the
smallest that tell the fields apart (H=3, nj=2, nobs=1, K=5, B=2).  No compute calls here (CPU)."""
import ctypes as C

import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib

H, NJ, NOBS, K, B = 3, 2, 1, 5, 2
NS, NN, NX = 2 * NJ, H * NJ, H * 2 * NJ
OUT8 = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")


class _Recorder:
    """stands in for the library: every call is recorded as (symbol, arguments) and succeeds; `hooks[symbol]` runs first"""

    def __init__(self, **hooks):
        self.calls, self.hooks = [], hooks

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in self.hooks:
                self.hooks[name](*args)
            return 0
        return call

    def only(self, name):
        hit = [a for n, a in self.calls if n == name]
        assert len(hit) == 1, [n for n, _ in self.calls]
        return hit[0]


class _Handle(pkg.CFSBatch):
    """a CFSBatch of the smallest shape with a recorder for a library"""
    obstacle_motion = "static"

    def __init__(self, meshes=()):
        self.H, self.nj, self.ns, self.nn, self.nx, self.nobs, self.K, self.max_batch = H, NJ, NS, NN, NX, NOBS, K, B
        self.rows = NOBS * H * (1 + 2 * NJ)
        self.margin = np.full(NOBS, 0.2)
        self._lib, self._h, self._meshes = _Recorder(), "handle", list(meshes)

    def close(self):
        pass

    __del__ = close


def _at(p):
    """the address a pointer argument holds (None for NULL)"""
    return p.value if isinstance(p, C.c_void_p) else p


def _same(p, a):
    assert _at(p) == a.ctypes.data and a.flags.c_contiguous


def _struct_is(struct, ns, names):
    """every pointer field of `struct` named in `names` is the address of ns.<name>; the other pointer fields are NULL"""
    for f, t in struct._fields_:
        if t is not C.c_void_p:
            continue
        if f in names:
            _same(getattr(struct, f), getattr(ns, f))
        else:
            assert getattr(struct, f) is None, f
    assert len({getattr(ns, f).ctypes.data for f in names}) == len(names)


def _inputs():
    r = np.random.default_rng(0)
    return dict(x_init=r.random((B, NX)), xR1=r.random((B, NS)), ff=r.random((B, NN)), caug=r.random(B), obs=r.random((B, NOBS, 6)))


def _check_out8(r):
    assert r.u.shape == (B, NN) and r.x_.shape == (B, NX) and r.cost_all.shape == r.e_cost_all.shape == r.e_u_all.shape == (B, K)
    assert r.iter_O.shape == r.total_iter.shape == r.status.shape == (B,)
    assert all(getattr(r, k).dtype == (np.int32 if k in OUT8[5:] else np.float64) for k in OUT8)


@pytest.mark.parametrize("rows", [None, 4])
def test_solve(rows):
    h, a = _Handle(), _inputs()
    noise = None if rows is None else np.random.default_rng(1).random((B, rows, NN))
    r = h.solve(a["x_init"], a["xR1"], a["ff"], a["caug"], a["obs"], noise=noise)
    hh, i, o = h._lib.only("cfs_solve_batch")
    i, o = i._obj, o._obj
    assert hh == "handle" and isinstance(i, _lib.cfs_batch_in) and isinstance(o, _lib.cfs_batch_out)
    assert i.B == B and i.noise_rows == (0 if rows is None else rows)
    for k, v in a.items():
        _same(getattr(i, k), v)
    if rows is None:
        assert i.noise is None
    else:
        _same(i.noise, noise)
    _struct_is(o, r, OUT8)
    _check_out8(r)
    hh, nb, viol, ns = h._lib.only("cfs_soft_results")
    assert (hh, nb) == ("handle", B)
    _same(viol, r.viol_all)
    _same(ns, r.n_soft)
    assert r.viol_all.shape == (B, K) and r.n_soft.dtype == np.int32 and r.n_soft.shape == (B,)
    assert [n for n, _ in h._lib.calls] == ["cfs_solve_batch", "cfs_soft_results"]


def test_chomp():
    h, a = _Handle(), _inputs()
    u0, D, eps = np.random.default_rng(2).random((B, NN)), np.array([0.3]), np.array([0.1])
    r = h.chomp(a["x_init"], a["xR1"], a["ff"], a["caug"], a["obs"], u0, D, eps)
    hh, i, pu0, pD, peps, o = h._lib.only("cfs_chomp_batch")
    i, o = i._obj, o._obj
    assert hh == "handle" and i.B == B and i.noise is None and i.noise_rows == 0
    for k, v in a.items():
        _same(getattr(i, k), v)
    _same(pu0, u0)
    _same(pD, D)
    _same(peps, eps)
    _struct_is(o, r, OUT8)
    _check_out8(r)
    assert len(h._lib.calls) == 1


AUDIT = ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path")


@pytest.mark.parametrize("mesh", [False, True])
def test_clearance(mesh):
    h, a = _Handle(meshes=[object()] if mesh else ()), _inputs()
    x_, u = a["x_init"], np.random.default_rng(3).random((B, NN))
    r = (h.clearance_mesh if mesh else h.clearance)(x_, u, a["xR1"], a["obs"], substeps=7)
    args = h._lib.only("cfs_clearance_mesh" if mesh else "cfs_clearance")
    names = AUDIT + (("tri_path",) if mesh else ())
    assert args[:3] == ("handle", B, 7) and len(args) == 7 + len(names) and len(h._lib.calls) == 1
    for p, v in zip(args[3:7], (x_, u, a["xR1"], a["obs"])):
        _same(p, v)
    for p, k in zip(args[7:], names):
        _same(p, getattr(r, k))
        assert getattr(r, k).shape == (B, NOBS) and getattr(r, k).dtype == (np.int32 if k in ("link_path", "tri_path") else np.float64)
    assert len({_at(p) for p in args[7:]}) == len(names)
    assert sorted(vars(r)) == sorted(names + ("short_by",))
    np.testing.assert_array_equal(r.short_by, np.full(B, 0.2))            # margin - dist_path with the recorder's zeros


def test_linearize_and_get_con():
    h, a = _Handle(), _inputs()
    dist, lid, grad = h.linearize(a["x_init"], a["obs"])
    args = h._lib.only("cfs_linearize")
    assert args[:2] == ("handle", B) and len(args) == 7
    for p, v in zip(args[2:], (a["x_init"], a["obs"], dist, lid, grad)):
        _same(p, v)
    assert dist.shape == lid.shape == (B, NOBS, H) and grad.shape == (B, NOBS, H, NJ) and lid.dtype == np.int32
    u = np.random.default_rng(4).random((B, NN))
    A, b = h.get_con(a["x_init"], u, a["xR1"], a["obs"])
    args = h._lib.only("cfs_get_con")
    assert args[:2] == ("handle", B) and len(args) == 8
    for p, v in zip(args[2:], (a["x_init"], u, a["xR1"], a["obs"], A.transpose(0, 2, 1), b)):
        _same(p, v)
    assert A.shape == (B, h.rows, NN) and b.shape == (B, h.rows)


@pytest.mark.parametrize("want_lambda", [True, False])
def test_qp(want_lambda):
    h, g = _Handle(), np.random.default_rng(5)
    lin, u_lin, xR1, dist, grad = g.random((B, NX)), g.random((B, NN)), g.random((B, NS)), g.random((B, NOBS, H)), g.random((B, NOBS, H, NJ))
    u, lam, it, st = h.qp(lin, u_lin, xR1, dist, grad, want_lambda=want_lambda)
    args = h._lib.only("cfs_qp")
    assert args[:2] == ("handle", B) and len(args) == 11
    for p, v in zip(args[2:8], (lin, u_lin, xR1, dist, grad, u)):
        _same(p, v)
    if want_lambda:
        _same(args[8], lam)
        assert lam.shape == (B, NOBS * H + 4 * NN)                        # the recorder leaves `on` at 0: no joint limits
    else:
        assert lam is None and _at(args[8]) is None
    _same(args[9], it)
    _same(args[10], st)
    assert u.shape == (B, NN) and it.dtype == st.dtype == np.int32 and it.shape == st.shape == (B,)


@pytest.mark.parametrize("want_u", [True, False])
def test_cost_b_and_get_cost(want_u):
    h, a = _Handle(), _inputs()
    got = h.cost_b(a["ff"], a["caug"], want_u=want_u)
    cost, ub = got if want_u else (got, None)
    args = h._lib.only("cfs_cost_b")
    assert args[:2] == ("handle", B) and len(args) == 6
    for p, v in zip(args[2:5], (a["ff"], a["caug"], cost)):
        _same(p, v)
    assert _at(args[5]) == (ub.ctypes.data if want_u else None) and cost.shape == (B,) and (ub is None or ub.shape == (B, NN))
    u = np.random.default_rng(6).random((B, NN))
    cost = h.get_cost(u, a["ff"], a["caug"])
    args = h._lib.only("cfs_get_cost")
    assert args[:2] == ("handle", B) and len(args) == 6
    for p, v in zip(args[2:], (u, a["ff"], a["caug"], cost)):
        _same(p, v)


def test_launch_order_debug():
    h, a = _Handle(), _inputs()
    key, order = h.launch_order_debug(a["x_init"], a["obs"])
    args = h._lib.only("cfs_debug_launch_order")
    assert args[:2] == ("handle", B) and len(args) == 6 and len(h._lib.calls) == 1
    for p, v in zip(args[2:], (a["x_init"], a["obs"], key, order)):
        _same(p, v)
    assert key.shape == order.shape == (B,) and key.dtype == order.dtype == np.int32 and key.ctypes.data != order.ctypes.data


# ---- the entries without a handle: _lib.lib is the recorder ------------------------------------------------------------------
IK7 = ("theta", "status", "selected", "n_ok", "err_pos", "err_axis", "clearance")
IK_CAND = ("cand_theta", "cand_status", "cand_iter")
CART7 = ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance")
CART_CAND = ("cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")


@pytest.mark.parametrize("want", [False, True])
def test_ik_solve(monkeypatch, want):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    T, R, nj = 2, 3, 5
    ik = pkg.IKSolver(pkg.robotproperty2("M200i"), restarts=R)
    r = ik.solve(np.zeros((T, 3)), target_axis=[0.0, 0.0, 1.0], seed=9, want_candidates=want)
    d, nT, tp, ta, tr, o = rec.only("cfs_ik_solve")
    d, o = d._obj, o._obj
    assert isinstance(d, _lib.cfs_ik_desc) and (d.njoint, d.use_axis, d.restarts, d.seed, d.nobs, nT) == (nj, 1, R, 9, 0, T)
    assert None not in (_at(tp), _at(ta), _at(tr)) and len(rec.calls) == 1
    names = IK7 + (IK_CAND if want else ())
    assert sorted(vars(r)) == sorted(names)
    _struct_is(o, r, names)
    shapes = dict(theta=(T, nj), cand_theta=(T, R, nj), cand_status=(T, R), cand_iter=(T, R))
    ints = ("status", "selected", "n_ok", "cand_status", "cand_iter")
    for k in names:
        assert getattr(r, k).shape == shapes.get(k, (T,)) and getattr(r, k).dtype == (np.int32 if k in ints else np.float64), k


@pytest.mark.parametrize("want", [False, True])
def test_cart_trace(monkeypatch, want):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    T, R, nj, steps = 2, 3, 5, 4
    cp = pkg.CartesianPath(pkg.robotproperty2("M200i"), steps=steps)
    r = cp.trace(np.zeros((T, R, nj)), np.zeros((T, 3)), start_state=np.zeros((T, R), int), want_candidates=want)
    d, nT, s, ss, tp, ta, tr, o = rec.only("cfs_cart_path")
    d, o = d._obj, o._obj
    assert isinstance(d, _lib.cfs_cart_desc) and (d.njoint, d.use_axis, d.candidates, d.steps, d.nobs, nT) == (nj, 0, R, steps, 0, T)
    assert None not in (_at(s), _at(ss), _at(tp), _at(tr)) and _at(ta) is None and len(rec.calls) == 1
    names = CART7 + (CART_CAND if want else ())
    assert sorted(vars(r)) == sorted(names)
    _struct_is(o, r, names)
    K1 = steps + 1
    shapes = dict(theta=(T, nj), path=(T, K1, nj), cand_status=(T, R), cand_done=(T, R), cand_iter=(T, R), cand_end=(T, R, nj),
                  cand_path=(T, R, K1, nj))
    floats = ("theta", "path", "clearance", "cand_end", "cand_path")
    for k in names:
        assert getattr(r, k).shape == shapes.get(k, (T,)) and getattr(r, k).dtype == (np.float64 if k in floats else np.int32), k


def test_rrt_grow(monkeypatch):
    """the recorder writes a different value through every pointer of cfs_rrt_out; each must come back under its own name"""
    S = 2

    def write(d, nS, o):
        o = o._obj
        put = lambda f, t, i, v: C.cast(getattr(o, f), C.POINTER(t)).__setitem__(i, v)  # noqa: E731
        N = pkg.RRT_FANUC.MAX_ITER + 1
        for t in range(nS):
            put("node_num", C.c_int32, t, 2)
            put("fail", C.c_int32, t, 3)
            put("route_len", C.c_int32, t, 1)
            put("draws_used", C.c_int64, t, 11 + t)
            put("proposals", C.c_int64, t, 21 + t)
            put("parent", C.c_int32, t * N + 1, 1)
            put("nodes", C.c_double, (t * N + 1) * 5, 0.125)
            put("total_dis", C.c_double, t * N + 1, 0.5)
            put("all_ee", C.c_double, t * pkg.RRT_FANUC.MAX_ITER * 3, 0.75)
            put("route", C.c_double, t * N * 5, 0.25)
    rec = _Recorder(cfs_rrt_grow=write)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    obs, s, goal, region_g, region_s, off = pkg.RRTstar_problem()
    out = pkg.RRT_FANUC(obs, s, goal, region_g, region_s, off, "M200i", "RRT").grow(seed=5, S=S, max_draws=77)
    d, nS, o = rec.only("cfs_rrt_grow")
    d, o = d._obj, o._obj
    assert isinstance(d, _lib.cfs_rrt_desc) and (nS, d.seed, d.max_draws, d.nobs, d.nstate, d.solver, d.uniforms) == (S, 5, 77, 2, 5, 0, None)
    assert all(getattr(o, f) is not None for f, _ in o._fields_) and len({getattr(o, f) for f, _ in o._fields_}) == len(o._fields_)
    assert len(out) == S and len(rec.calls) == 1
    for t, r in enumerate(out):
        assert (r.node_num, r.fail, r.fail_code, r.draws_used, r.proposals) == (2, True, 3, 11 + t, 21 + t)
        assert r.route.shape == (5, 1) and r.route[0, 0] == 0.25
        assert r.all_nodes.shape == (6, 2) and r.all_nodes[0, 1] == 1.0 and r.all_nodes[1, 1] == 0.125
        assert r.total_dis.tolist() == [0.0, 0.5] and r.all_ee.shape == (3, 1) and r.all_ee[0, 0] == 0.75
