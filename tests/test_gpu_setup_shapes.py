"""The kernels that prepare a batch and evaluate its cost, each against the plain longdouble reference of tests/setup_reference.py
at tile edges and at every joint count: cfs_batched_gemv_kernel and cfs_cost_history_kernel (get_cost, cost_b, the cost history of
a CFS solve), cfs_build_terms_kernel (line reference, route resampling, ff, caug, xR1), cfs_dense_con_kernel (get_con) and the
launch-order pre-pass (cfs_order_key_kernel, cfs_order_rank_kernel through cfs_debug_launch_order).  Every bound is derived from
the arithmetic the kernel's comments describe, with EPS = 2^-52 and gamma(m) = m EPS / (1 - m EPS); each test prints the worst
observed error over its bound.  Handles are created through the dense path (use_weights=False)."""
import copy

import numpy as np
import pytest

from motionplanning_5d_m_amd.sysinfo import cost_terms

import setup_reference as R

pytestmark = pytest.mark.gpu

EPS, LD = R.EPS, R.LD
# (nj, H): nn below one 16-row tile, on it, on the 32 rows of one wavefront, one past it, across two and three wavefronts
SHAPES = [(2, 1), (3, 1), (5, 1), (5, 3), (4, 4), (2, 16), (4, 8), (3, 11), (6, 6), (5, 13)]
BATCHES = (1, 15, 16, 17, 33)                   # below, on, across and twice across the 16-problem tile
X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])


def _robot_name(nj):
    return "2L" if nj == 2 else "M200i"


def _family(gpu, nj, H, K=3, epsilon_O=0.1, seed=0):
    """a problem family of the first nj joints of the M200i (the 2L arm for nj = 2) with the drivers' kind of weights"""
    rng = np.random.default_rng(1000 * nj + H + seed)
    robot = gpu.robotproperty2(_robot_name(nj))
    x0, xg = rng.uniform(-1, 1, nj), rng.uniform(-1, 1, nj)
    w = np.array([10.0, 10, 1, 1, 1, 1])[:nj]
    kw = dict(Qp=np.diag(w), Qv=np.diag(w), Rblk=np.eye(nj) * 2 + 0.25 * (np.eye(nj, k=1) + np.eye(nj, k=-1)), cR=50.0,
              lim=1.0 - 0.05 * np.arange(nj), max_input_blk=np.ones(nj), epsilon_O=epsilon_O, MAX_O_ITER=K)
    return gpu.build_sys_info(robot, nj, H, x0, xg, gpu.line_reference(x0, xg, H), **kw)


def _handle(gpu, s, nobs=1, margin=(0.2,), mode="CFS", max_batch=1, **kw):
    return gpu.CFSBatch(s, nobs, list(margin), mode=mode, max_batch=max_batch, use_weights=False, **kw)


def _terms(s, x0, xg):
    """(xR1, ff, caug) of B (start, goal) pairs from the float64 host builder"""
    nj, H = s.njoint, s.H
    xR1 = np.concatenate([x0, np.zeros_like(x0)], axis=1)
    fc = [cost_terms(s.Aaug, s.Baug, s.Qaug_state, xR1[b], xg[b], H, nj) for b in range(x0.shape[0])]
    return xR1, np.stack([f for f, _ in fc]), np.array([c for _, c in fc])


def _obstacles(rng, robot, shape):
    """random line obstacles (shape + (6,)) within the arm's reach"""
    if robot.name == "2L":
        lo, hi = np.array([-0.5, -0.5, -0.1]), np.array([0.5, 0.5, 0.1])
    else:
        lo, hi = np.asarray(robot.base) + np.array([-0.7, -0.7, -0.2]), np.asarray(robot.base) + np.array([0.7, 0.7, 1.0])
    return np.concatenate([rng.uniform(lo, hi, shape + (3,)), rng.uniform(lo, hi, shape + (3,))], axis=-1)


# ---- a. the matrix-core product, exact ---------------------------------------------------------------------------------------
def integer_qq(nn, rng):
    """G'G + diag(s), G in -3..3, s >= nn chosen so that the diagonal is strictly increasing and above every off-diagonal entry:
    symmetric, positive definite, integers below 2^10"""
    G = rng.integers(-3, 4, (nn, nn)).astype(np.float64)
    GG = G.T @ G
    QQ = GG + np.diag(GG.diagonal().max() + nn + np.arange(nn) - GG.diagonal())
    assert (QQ == QQ.T).all() and np.abs(QQ).max() < 2 ** 10 and (QQ.diagonal() - GG.diagonal() >= nn).all()
    return QQ


@pytest.mark.parametrize("nj,H", SHAPES)
def test_matrix_core_product_is_exact_on_integers(gpu, nj, H):
    """Integer QQ, u, ff, caug: every product and partial sum of QQ u (MFMA), u'(QQ u), ff'u and of the final 0.5 quad + lin + caug is
    an integer or half-integer far below 2^53, whatever the order of summation, so get_cost equals the longdouble value bit for bit.

    Lane-to-element map: u = e_c for every c at B = nn gives 0.5 QQ[c, c] + ff[c] + caug.  A wrong pairing of an output row or of an
    operand element would put another entry QQ[r, c'] in the place of QQ[c, c], so the probe is not vacuous exactly when every
    diagonal entry differs from every other entry of the matrix; that is asserted (all nn^2 entries cannot be distinct: the matrix is
    symmetric, and nn^2 > 2^11 at nn = 65).  u = e_r + e_c for every r < c then reads each off-diagonal pair, QQ[r, c] + QQ[c, r]."""
    nn = nj * H
    rng = np.random.default_rng(nn * 7 + nj)
    s = copy.copy(_family(gpu, nj, H))
    s.QQ = integer_qq(nn, rng)
    diag, off = s.QQ.diagonal(), s.QQ[~np.eye(nn, dtype=bool)]
    assert np.unique(diag).size == nn and not np.isin(diag, off).any()
    pairs = [(r, c) for r in range(nn) for c in range(r + 1, nn)]
    Bmax = max(max(BATCHES), nn, len(pairs))
    for mode in ("CFS", "PSGCFS"):
        slv = _handle(gpu, s, mode=mode, max_batch=Bmax)
        for B in BATCHES:
            u = rng.integers(-8, 9, (B, nn)).astype(np.float64)
            ff = rng.integers(-8, 9, (B, nn)).astype(np.float64)
            caug = rng.integers(-100, 101, B).astype(np.float64)
            want = R.gemv_cost(s.QQ, u, ff, caug)
            got = slv.get_cost(u, ff, caug)
            assert (got.astype(LD) == want).all(), (mode, B, np.nonzero(got.astype(LD) != want)[0])
            assert (slv.get_cost(np.zeros((B, nn)), ff, caug) == caug).all(), (mode, B)          # get_cost(0) = caug
        ff, caug = rng.integers(-8, 9, (nn, nn)).astype(np.float64), rng.integers(-100, 101, nn).astype(np.float64)
        got = slv.get_cost(np.eye(nn), ff, caug)
        assert (got == 0.5 * diag + ff.diagonal() + caug).all(), (mode, np.nonzero(got != 0.5 * diag + ff.diagonal() + caug)[0])
        if pairs:
            u = np.zeros((len(pairs), nn))
            for n, (r, c) in enumerate(pairs):
                u[n, r] = u[n, c] = 1.0
            z = np.zeros(len(pairs))
            want = np.array([0.5 * (s.QQ[r, r] + s.QQ[c, c] + s.QQ[r, c] + s.QQ[c, r]) for r, c in pairs])
            assert (slv.get_cost(u, np.zeros_like(u), z) == want).all(), mode
        slv.close()


# ---- b. cost_b ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj,H", SHAPES)
def test_cost_b_against_the_longdouble_solve(gpu, nj, H):
    """u_b = -H^-1 ff (H = QQ symmetrised) on the real family matrices against the longdouble Cholesky solve.  Margin, taken at run
    time: the error of float64 -(inv(Hs) @ ff) against the same longdouble solution on the same inputs, times 8 (the device does
    the same product with a host-computed inverse; 8 covers another summation order and the Cholesky-built inverse), floor
    nn EPS max|u*|.  cost_b against the reference's cost at its own minimiser: the rounding of get_cost at u_b (the bound of the
    cost-history test) plus what the error of u_b is worth, |grad*|'|d| + 0.5 |d|'|Hs||d| with |d| <= the margin above."""
    nn = nj * H
    s = _family(gpu, nj, H)
    rng = np.random.default_rng(nn)
    Bm = max(BATCHES)
    _, ff, caug = _terms(s, rng.uniform(-1, 1, (Bm, nj)), rng.uniform(-1, 1, (Bm, nj)))
    Hs = 0.5 * (s.QQ + s.QQ.T)
    ustar = R.solve_ld(Hs, -ff.T).T                                                    # (Bm, nn)
    u64 = -(np.linalg.inv(Hs) @ ff.T).T
    tol = np.maximum(8 * np.abs(u64 - ustar).max(axis=1), nn * EPS * np.abs(ustar).max(axis=1)).astype(np.float64)
    cstar = R.gemv_cost(s.QQ, ustar, ff, caug)
    gstar = np.abs(ustar @ R.ld(Hs) + ff)                                              # the gradient at u*: rounding of the solve only
    second = gstar.sum(axis=1) * tol + 0.5 * tol * tol * np.abs(Hs).sum()
    worst_u = worst_c = 0.0
    for mode in ("CFS", "PSGCFS"):
        slv = _handle(gpu, s, mode=mode, max_batch=Bm)
        for B in BATCHES:
            cb, ub = slv.cost_b(ff[:B], caug[:B], want_u=True)
            ru = np.abs(ub - ustar[:B]).max(axis=1) / tol[:B]
            bound = R.gamma(nn + 2) * R.gemv_cost_abs(s.QQ, ub, ff[:B], caug[:B]) + second[:B]
            rc = np.abs(cb - cstar[:B]) / bound
            worst_u, worst_c = max(worst_u, float(ru.max())), max(worst_c, float(rc.max()))
            assert (ru <= 1).all(), (mode, B, ru.max())
            assert (rc <= 1).all(), (mode, B, rc.max())
            assert (cb == slv.cost_b(ff[:B], caug[:B])).all()                          # with and without u_b returned
        slv.close()
    print(f"\ncost_b nj={nj} H={H} nn={nn}: worst |u_b - u*| / margin = {worst_u:.3f}, worst |cost_b - cost*| / bound = {worst_c:.3f}")


# ---- c. cost history of a CFS solve -------------------------------------------------------------------------------------------
HISTORY_B = 17


def history_case(pkg, nj, H, K):
    """17 problems of the first nj joints of the M200i that sweep joint 1 past a line obstacle (a single waypoint: poses around it),
    so that some of them iterate: (sys_info, x_init, xR1, ff, caug, obs, margin).  The three-joint arm is shorter: its obstacle
    stands closer and has a wider margin.  The seeds were checked with the CPU oracle: at MAX_O_ITER = 6 every shape has problems
    with 3 or more iterates, and problems whose first or a later QP is infeasible."""
    s = _family(pkg, nj, H, K=K, epsilon_O=1e-4)
    rng = np.random.default_rng(100 * nj + H)
    B = HISTORY_B
    x0 = X0[:nj] + 0.15 * rng.standard_normal((B, nj))
    xg = X0[:nj] * np.array([-1.0, 1, 1, 1, 1, 1])[:nj] + 0.15 * rng.standard_normal((B, nj))
    if H == 1:
        xg[:, 0] = rng.uniform(-0.45, 0.45, B)
    x_init = np.stack([pkg.line_reference(x0[b], xg[b], H) for b in range(B)])
    xR1, ff, caug = _terms(s, x0, xg)
    ox, margin = (3550, 0.3) if nj == 3 else (3700, 0.2)
    ob = pkg.obs_to_array([pkg.cylinder((ox, 8500, 1), (ox, 8500, 1200), 0.15, margin)])
    obs = ob[None] + np.concatenate([0.04 * rng.standard_normal((B, 1, 2)), np.zeros((B, 1, 1))] * 2, axis=2)
    return s, x_init, xR1, ff, caug, obs, margin


@pytest.mark.parametrize("K", [1, 2, 6])
@pytest.mark.parametrize("nj,H", [(5, 1), (3, 11), (5, 13)])
def test_cost_history_is_the_cost_of_every_logged_iterate(gpu, nj, H, K):
    """cost_all[b, k] is get_cost of iterate k (the u the solver logged), e_cost_all the difference of consecutive costs.
    Rounding of 0.5 u'(QQ u) + ff'u + caug in any order of summation: nn products and nn - 1 additions per row of QQ u, then the
    same for the two dots, the halving and two additions, all against the sum of absolute values; gamma(nn + 2) with EPS = 2 u
    covers the 2 nn + 4 roundings."""
    nn = nj * H
    s, x_init, xR1, ff, caug, obs, margin = history_case(gpu, nj, H, K)
    B = HISTORY_B
    slv = _handle(gpu, s, margin=(margin,), max_batch=B)
    slv.log_u(True)
    r = slv.solve(x_init, xR1, ff, caug, obs)
    ulog = slv.read_u_log(B)
    slv.close()
    n_it = r.iter_O - 1
    assert (n_it >= 0).all() and (n_it <= K).all()
    if K == 6:
        assert n_it.max() >= 3, n_it
    worst = 0.0
    for b in range(B):
        n = int(n_it[b])
        prev = caug[b]
        for k in range(n):
            ref = R.gemv_cost(s.QQ, ulog[b, k], ff[b], caug[b])[0]
            bound = R.gamma(nn + 2) * R.gemv_cost_abs(s.QQ, ulog[b, k], ff[b], caug[b])[0]
            err = abs(LD(r.cost_all[b, k]) - ref)
            worst = max(worst, float(err / bound))
            assert err <= bound, (b, k, float(err), float(bound))
            assert r.e_cost_all[b, k] == abs(prev - r.cost_all[b, k]), (b, k)
            prev = r.cost_all[b, k]
        assert (r.cost_all[b, n:] == 0).all() and (r.e_cost_all[b, n:] == 0).all(), b
        if n >= 1:
            assert (ulog[b, n - 1] == r.u[b]).all(), b
    print(f"\ncost history nj={nj} H={H} nn={nn} K={K}: iterates logged {np.bincount(n_it, minlength=K + 1).tolist()}, "
          f"worst |cost_all - ref| / bound = {worst:.3f}")


# ---- d. terms builder -----------------------------------------------------------------------------------------------------------
LINE_H = (1, 2, 7, 33)
ROUTES = ((2, 1), (2, 7), (3, 4), (5, 8), (12, 5), (9, 33))   # (nwp, H): knots on samples, more waypoints than samples, generic
RAGGED_STRIDE, RAGGED_H = 12, 8
RAGGED_LEN = (1, 2, 3, 12, 7, 5, 9, 4, 6, 8, 10, 11, 1, 2, 12, 3, 7)


def _check_cost_terms(s, xR1, xg, ff, caug, tag):
    """ff and caug of every problem within gamma(2 H ns + nj + 2) of the componentwise absolute sums; returns the worst ratios"""
    nj, H = s.njoint, s.H
    g = R.gamma(2 * H * 2 * nj + nj + 2)
    wf = wc = 0.0
    for b in range(xR1.shape[0]):
        f, c, S, Sc = R.cost_terms_ld(s.Aaug, s.Baug, s.Qaug_state, xR1[b], xg[b])
        ef, ec = np.abs(ff[b] - f), abs(caug[b] - c)
        assert (ef <= g * S).all(), (tag, b, float((ef / (g * S)).max()))
        assert ec <= g * Sc, (tag, b, float(ec / (g * Sc)))
        wf, wc = max(wf, float((ef / (g * S)).max())), max(wc, float(ec / (g * Sc)))
    return wf, wc


@pytest.mark.parametrize("nj", [2, 3, 4, 5, 6])
def test_terms_builder(gpu, nj):
    """cfs_build_terms_kernel for (start, goal) pairs, routes and ragged routes.
    Line: x0 + (i+1) ((xg - x0) / H) within 2 EPS max(|x0|, |xg|) per joint, the last waypoint xg itself.
    Routes: per entry EPS (4 max|r| + 2 nwp |r_k+1 - r_k|): the final rounding, and the cancellation in tau = (t - t0) / (t1 - t0)
    with t up to (nwp - 1) dt; at a knot either neighbouring segment may be named and the value is the knot.
    ff, caug: two nested dot products of length H ns on the host (in long double, rounded once) and one of length nj (2 nj by
    2 nj for caug) in the kernel, against S = |Baug'| |Qaug| (|Aaug| |xR1| + |gaug|) and its caug analogue: gamma(2 H ns + nj + 2)."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev).contiguous()  # noqa: E731
    host = lambda vs: [v.cpu().numpy() for v in vs]  # noqa: E731
    rng = np.random.default_rng(nj)
    B = 3
    handles = {}

    def handle(H):
        if H not in handles:
            s = _family(gpu, nj, H)
            handles[H] = (s, _handle(gpu, s, max_batch=len(RAGGED_LEN)))
            handles[H][1].set_state_cost(s.Qaug_state)
        return handles[H]

    w_line = w_route = w_ff = w_c = 0.0
    for H in LINE_H:
        s, slv = handle(H)
        x0, xg = rng.uniform(-2, 2, (B, nj)), rng.uniform(-2, 2, (B, nj))
        x_init, xR1, ff, caug = host(slv.build_terms_device(t(x0), t(xg)))
        for b in range(B):
            want, wx1 = R.line_terms(x0[b], xg[b], H)
            got = x_init[b].reshape(H, 2 * nj)
            bound = 2 * EPS * np.maximum(np.abs(x0[b]), np.abs(xg[b]))
            err = np.abs(got[:, :nj] - want[:, :nj])
            assert (err <= bound).all(), (H, b, float((err / bound).max()))
            w_line = max(w_line, float((err / bound).max()))
            assert (got[-1, :nj] == xg[b]).all() and (got[:, nj:] == 0).all() and not np.signbit(got[:, nj:]).any()
            assert (xR1[b] == wx1).all() and not np.signbit(xR1[b, nj:]).any()
        a, c = _check_cost_terms(s, xR1, xg, ff, caug, ("line", H))
        w_ff, w_c = max(w_ff, a), max(w_c, c)
    for nwp, H in ROUTES:
        s, slv = handle(H)
        routes = rng.uniform(-2, 2, (B, nwp, nj))
        x_init, xR1, ff, caug = host(slv.build_terms_from_routes_device(t(routes)))
        for b in range(B):
            want, wx1, seg = R.route_terms(routes[b], nwp, s.robot.delta_t, H)
            got = x_init[b].reshape(H, 2 * nj)
            bound = EPS * (4 * np.abs(routes[b]).max(axis=0)[None, :] + 2 * nwp * seg)
            err = np.abs(got[:, :nj] - want[:, :nj])
            assert (err <= bound).all(), (nwp, H, b, float((err / bound).max()))
            w_route = max(w_route, float((err / bound).max()))
            assert (got[:, nj:] == 0).all() and (xR1[b] == wx1).all()
        a, c = _check_cost_terms(s, xR1, routes[:, -1], ff, caug, ("route", nwp, H))
        w_ff, w_c = max(w_ff, a), max(w_c, c)
    # ragged routes: rows at or past each length are NaN and must not be read
    s, slv = handle(RAGGED_H)
    H, Bn = RAGGED_H, len(RAGGED_LEN)
    routes = rng.uniform(-2, 2, (Bn, RAGGED_STRIDE, nj))
    for b, n in enumerate(RAGGED_LEN):
        routes[b, n:] = np.nan
    x_init, xR1, ff, caug = host(slv.build_terms_from_ragged_routes_device(t(routes), t(np.array(RAGGED_LEN), torch.int32)))
    assert not (np.isnan(x_init).any() or np.isnan(xR1).any() or np.isnan(ff).any() or np.isnan(caug).any())
    for b, n in enumerate(RAGGED_LEN):
        want, wx1, seg = R.route_terms(routes[b], n, s.robot.delta_t, H)
        got = x_init[b].reshape(H, 2 * nj)
        if n == 1:                                                                       # start = goal: stay there
            assert (got[:, :nj] == routes[b, 0]).all()
        bound = EPS * (4 * np.abs(routes[b, :n]).max(axis=0)[None, :] + 2 * n * seg)
        err = np.abs(got[:, :nj] - want[:, :nj])
        assert (err <= bound).all(), ("ragged", b, n, float((err / bound).max()))
        w_route = max(w_route, float((err / bound).max()))
        assert (got[:, nj:] == 0).all() and (xR1[b] == wx1).all()
    xg = np.stack([routes[b, n - 1] for b, n in enumerate(RAGGED_LEN)])
    a, c = _check_cost_terms(s, xR1, xg, ff, caug, "ragged")
    w_ff, w_c = max(w_ff, a), max(w_c, c)
    for _, slv in handles.values():
        slv.close()
    print(f"\nterms builder nj={nj}: worst error / bound: line {w_line:.3f}, routes {w_route:.3f}, ff {w_ff:.3f}, caug {w_c:.3f}")


# ---- e. dense constraint writer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [2, 3, 4, 6])
def test_dense_constraint_writer(gpu, nj):
    """get_con against the reference built from the SAME handle's linearize output, so that only the writer is under test, at
    u != 0 with a moving start and distinct margins and velocity limits; then with joint limits whose first lo and last hi are
    infinite.  Collision entries -(g coef dt dt): three roundings, 3 EPS.  Collision binq (d - margin) - sum_c g_c (sum_k coef u):
    (i + 1) nj products and sums and three more roundings against the absolute sum, gamma((i + 1) nj + 3).  The other rows of binq
    are one or two operations: 2 EPS of their absolute sum."""
    rng = np.random.default_rng(10 + nj)
    B = 3
    worst_a = worst_b = worst_v = 0.0
    for H in (1, 2, 33):
        for nobs in (1, 3):
            nn, per = H * nj, 1 + 2 * nj
            rref = nobs * H * per
            s = _family(gpu, nj, H)
            margin = 0.1 + 0.07 * np.arange(nobs)
            slv = _handle(gpu, s, nobs=nobs, margin=margin, max_batch=B)
            x_ = rng.uniform(-1, 1, (B, H * 2 * nj))
            u = rng.uniform(-0.5, 0.5, (B, nn))
            xR1 = np.concatenate([rng.uniform(-1, 1, (B, nj)), rng.uniform(-0.2, 0.2, (B, nj))], axis=1)
            obs = _obstacles(rng, s.robot, (B, nobs))
            dist, _, grad = slv.linearize(x_, obs)
            assert np.abs(grad).max() > 1e-3 and (np.abs(u) > 0).all() and (xR1[:, nj:] != 0).all()
            lo, hi = -2.0 - 0.1 * np.arange(nj), 2.0 + 0.1 * np.arange(nj)
            lo[0], hi[-1] = -np.inf, np.inf
            coll = np.zeros(rref + 2 * nn, bool)
            coll[:rref:per] = True
            iwp = (np.arange(rref) // per) % H                                         # waypoint of a reference row
            for plim in (None, (lo, hi)):
                slv.set_joint_limits(None if plim is None else np.stack(plim, axis=1))
                rows = rref + (0 if plim is None else 2 * nn)
                assert slv.rows == rows
                A, b = slv.get_con(x_, u, xR1, obs)
                assert A.shape == (B, rows, nn) and b.shape == (B, rows)
                assert not np.signbit(A[A == 0]).any()
                for p in range(B):
                    Ar, br, babs = R.dense_con(dist[p], grad[p], margin, s.lim, plim, xR1[p], u[p], s.robot.delta_t, H, nj, nobs)
                    c = coll[:rows]
                    assert (A[p][~c].astype(LD) == Ar[~c]).all(), (H, nobs, p)
                    ea = np.abs(A[p][c] - Ar[c])
                    assert (ea <= 3 * EPS * np.abs(Ar[c])).all(), (H, nobs, p)
                    nz = Ar[c] != 0
                    if nz.any():                                                       # a link that ends at the fixed base has no gradient
                        worst_a = max(worst_a, float((ea[nz] / (3 * EPS * np.abs(Ar[c][nz]))).max()))
                    fin = np.isfinite(br.astype(np.float64))
                    assert (b[p][~fin] == br[~fin].astype(np.float64)).all() and (b[p][~fin] == np.inf).all()
                    with np.errstate(invalid="ignore"):                                # inf - inf in the rows checked just above
                        eb = np.abs(b[p] - br)
                    gb = np.array([R.gamma((i + 1) * nj + 3) for i in iwp[::per]]) * babs[:rref:per]
                    assert (eb[:rref:per] <= gb).all(), (H, nobs, p, float((eb[:rref:per] / gb).max()))
                    worst_b = max(worst_b, float((eb[:rref:per] / gb).max()))
                    other = ~c & fin
                    assert (eb[other] <= 2 * EPS * babs[other]).all(), (H, nobs, p)
                    worst_v = max(worst_v, float((eb[other] / (2 * EPS * babs[other])).max()))
                if plim is not None:
                    assert np.isinf(b).sum() == B * 2 * H                              # joint 0's lo rows and the last joint's hi rows
            slv.close()
            if (H, nj, nobs) == (33, 6, 3):
                assert rref > 256                                                      # more rows in a column than the workgroup has threads
            if (H, nj, nobs) == (1, 2, 1):
                assert rref == 5
    print(f"\ndense constraints nj={nj}: worst error / bound: collision Ainq {worst_a:.3f}, collision binq {worst_b:.3f}, "
          f"velocity and position binq {worst_v:.3f}")


# ---- f. launch order ---------------------------------------------------------------------------------------------------------------
def _line_keys(O, name, nj, x_init, obs_rows, margin):
    """reference keys: O.dist_arm pair by pair.  x_init (B, H, 2nj); obs_rows(b, i) -> (nline, 6) rows measured at waypoint i.
    Returns (key, smallest |d - margin_j| over the pairs)."""
    robot = O.robotproperty2(name)
    B, H = x_init.shape[:2]
    d = np.zeros((B, H, len(margin)))
    for b in range(B):
        for i in range(H):
            for j, row in enumerate(obs_rows(b, i)):
                d[b, i, j] = O.dist_arm(robot, x_init[b, i, :nj], np.stack([row[:3], row[3:]], axis=1))[0]
    return R.order_keys(d, margin), float(np.abs(d - np.asarray(margin)[None, None, :]).min())


def _check_order(key, order):
    assert sorted(order.tolist()) == list(range(len(key)))
    assert (order == R.stable_rank(key)).all()


ORDER_MARGIN = (0.05, 0.4)


@pytest.mark.parametrize("nj", [2, 5, 6])
def test_launch_order_keys_and_rank(gpu, O, nj):
    """static handles, two line obstacles with margins (0.05, 0.4): H below, on and across the 32 lanes a problem gets, B below, on
    and across the 8 problems of a workgroup"""
    rng = np.random.default_rng(20 + nj)
    name, Bm = _robot_name(nj), 41
    for H in (1, 31, 32, 33):
        s = _family(gpu, nj, H)
        slv = _handle(gpu, s, nobs=2, margin=ORDER_MARGIN, max_batch=Bm)
        x_init = np.concatenate([rng.uniform(-1.2, 1.2, (Bm, H, nj)), np.zeros((Bm, H, nj))], axis=2)
        obs = _obstacles(rng, s.robot, (Bm, 2))
        want, gap = _line_keys(O, name, nj, x_init, lambda b, i: obs[b], ORDER_MARGIN)
        assert gap > 1e-9, gap
        assert 0 < want.max() and (H == 1 or np.unique(want).size > 2)
        for B in (1, 7, 8, 9, 41):
            key, order = slv.launch_order_debug(x_init[:B].reshape(B, -1), obs[:B])
            assert (key == want[:B]).all(), (H, B, key, want[:B])
            _check_order(key, order)
        slv.close()


def test_launch_order_per_waypoint_handle(gpu, O):
    """obstacles that move across the horizon: waypoint i is measured against its own row i"""
    nj, H, B = 5, 33, 9
    rng = np.random.default_rng(31)
    s = _family(gpu, nj, H)
    slv = _handle(gpu, s, nobs=2, margin=ORDER_MARGIN, max_batch=B, obstacles="per_waypoint")
    x_init = np.concatenate([rng.uniform(-1.2, 1.2, (B, H, nj)), np.zeros((B, H, nj))], axis=2)
    a, z = _obstacles(rng, s.robot, (B, 2)), _obstacles(rng, s.robot, (B, 2))
    w = (np.arange(H) / (H - 1))[None, :, None, None]
    obs = a[:, None] * (1 - w) + z[:, None] * w                                        # (B, H, 2, 6)
    want, gap = _line_keys(O, "M200i", nj, x_init, lambda b, i: obs[b, i], ORDER_MARGIN)
    frozen, gap0 = _line_keys(O, "M200i", nj, x_init, lambda b, i: obs[b, 0], ORDER_MARGIN)
    assert gap > 1e-9 and gap0 > 1e-9 and (want != frozen).any()
    key, order = slv.launch_order_debug(x_init.reshape(B, -1), obs)
    slv.close()
    assert (key == want).all(), (key, want)
    _check_order(key, order)


def test_launch_order_skips_mesh_rows(gpu, O):
    """nobs = 3 whose last obstacle is a mesh (a small triangle far away): its row of obs holds a segment through the robot's base,
    which a line obstacle with the mesh's margin would count at every waypoint; margin[0..1] apply to the two lines"""
    nj, H, B = 5, 33, 9
    rng = np.random.default_rng(32)
    s = _family(gpu, nj, H)
    margin = ORDER_MARGIN + (5.0,)
    slv = _handle(gpu, s, nobs=3, margin=margin, max_batch=B)
    mesh = gpu.Mesh(tri=np.array([[[100.0, 100, 100], [100.1, 100, 100], [100, 100.1, 100]]]))
    slv.set_meshes([mesh])
    x_init = np.concatenate([rng.uniform(-1.2, 1.2, (B, H, nj)), np.zeros((B, H, nj))], axis=2)
    base = np.asarray(s.robot.base, float)
    through = np.concatenate([base - [0, 0, 1.0], base + [0, 0, 1.0]])
    obs = np.concatenate([_obstacles(rng, s.robot, (B, 2)), np.broadcast_to(through, (B, 1, 6))], axis=1)
    want, gap = _line_keys(O, "M200i", nj, x_init, lambda b, i: obs[b, :2], ORDER_MARGIN)
    as_line, _ = _line_keys(O, "M200i", nj, x_init, lambda b, i: obs[b], margin)
    assert gap > 1e-9 and (as_line == want + H).all()
    key, order = slv.launch_order_debug(x_init.reshape(B, -1), obs)
    assert (key == want).all(), (key, want)
    _check_order(key, order)
    slv.close()
    # a handle with no line obstacle at all: zero keys, the identity order
    only = _handle(gpu, s, nobs=1, margin=(5.0,), max_batch=B)
    only.set_meshes([mesh])
    key, order = only.launch_order_debug(x_init.reshape(B, -1), obs[:, 2:])
    assert (key == 0).all() and (order == np.arange(B)).all()
    only.close()
    mesh.close()


def test_launch_order_all_ties_two_rank_blocks(gpu, O):
    """B = 301, H = 1, one obstacle: keys are 0 or 1, every rank is a tie, and the rank kernel runs two workgroups"""
    nj, H, B = 5, 1, 301
    rng = np.random.default_rng(33)
    s = _family(gpu, nj, H)
    slv = _handle(gpu, s, nobs=1, margin=(0.4,), max_batch=B)
    x_init = np.concatenate([rng.uniform(-1.2, 1.2, (B, H, nj)), np.zeros((B, H, nj))], axis=2)
    obs = _obstacles(rng, s.robot, (B, 1))
    want, gap = _line_keys(O, "M200i", nj, x_init, lambda b, i: obs[b], (0.4,))
    assert gap > 1e-9 and sorted(np.unique(want).tolist()) == [0, 1] and min((want == 0).sum(), (want == 1).sum()) > 20
    key, order = slv.launch_order_debug(x_init.reshape(B, -1), obs)
    slv.close()
    assert (key == want).all()
    _check_order(key, order)
    assert (np.diff(order[:int((key == 1).sum())]) > 0).all() and (np.diff(order[int((key == 1).sum()):]) > 0).all()
