"""The longdouble references of tests/setup_reference.py against the project's float64 host builders (sysinfo.cost_terms,
line_reference, cubic_resample) and against the CPU oracle's get_con at a non-zero linearisation point.  What the GPU tests of
tests/test_gpu_setup_shapes.py measure the kernels against is checked here first, without a device (CPU)."""
import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd.sysinfo import cost_terms, cubic_resample, double_integrator, line_reference

import setup_reference as R

EPS = R.EPS


def _family(nj, H, seed=0):
    rng = np.random.default_rng(seed)
    robot = pkg.robotproperty2("2L" if nj == 2 else "M200i")
    x0, xg = rng.uniform(-1, 1, nj), rng.uniform(-1, 1, nj)
    kw = dict(Qp=np.diag(rng.uniform(1, 10, nj)), Qv=np.diag(rng.uniform(1, 10, nj)), Rblk=np.eye(nj) * 2 + 0.1, cR=10.0, lim=np.ones(nj),
              max_input_blk=np.ones(nj), epsilon_O=0.1, MAX_O_ITER=3)
    return pkg.build_sys_info(robot, nj, H, x0, xg, line_reference(x0, xg, H), **kw), x0, xg


def test_longdouble_is_wider_than_double():
    """the references are only references where long double carries more than 53 bits (x87: 64)"""
    assert np.finfo(R.LD).nmant > np.finfo(np.float64).nmant


@pytest.mark.parametrize("nj,H", [(2, 1), (3, 11), (5, 13), (6, 6)])
def test_gemv_cost_and_cost_terms(nj, H):
    s, x0, xg = _family(nj, H, seed=nj * 100 + H)
    nn = nj * H
    rng = np.random.default_rng(1)
    u, ff, caug = rng.standard_normal((4, nn)), rng.standard_normal((4, nn)), rng.standard_normal(4)
    want = 0.5 * np.einsum("bi,ij,bj->b", u, s.QQ, u) + (ff * u).sum(1) + caug
    got, scale = R.gemv_cost(s.QQ, u, ff, caug), R.gemv_cost_abs(s.QQ, u, ff, caug)
    assert (np.abs(got - want) <= R.gamma(nn + 2) * scale).all()
    assert (R.gemv_cost(s.QQ, np.zeros((4, nn)), ff, caug) == caug).all()
    xR1 = np.concatenate([x0, rng.standard_normal(nj) * 0.1])                        # a moving start: Aaug's velocity columns count
    f64, c64 = cost_terms(s.Aaug, s.Baug, s.Qaug_state, xR1, xg, H, nj)
    f, c, S, Sc = R.cost_terms_ld(s.Aaug, s.Baug, s.Qaug_state, xR1, xg)
    g = R.gamma(2 * H * 2 * nj + 2)
    assert (np.abs(f - f64) <= g * S).all() and abs(c - c64) <= g * Sc
    assert (S >= np.abs(f)).all() and Sc >= abs(c) and c >= 0
    # the unconstrained minimiser: the longdouble Cholesky solve against numpy's
    Hs = 0.5 * (s.QQ + s.QQ.T)
    x = R.solve_ld(Hs, -f64)
    ref = -np.linalg.solve(Hs, f64)
    assert np.abs(R.ld(Hs) @ x + f64).max() <= 1e-17 * np.abs(Hs).max() * np.abs(x).max() * nn
    assert np.abs(x - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("nj", [2, 3, 4, 5, 6])
def test_line_and_route_terms(nj):
    rng = np.random.default_rng(nj)
    for H in (1, 2, 7, 33):
        x0, xg = rng.uniform(-2, 2, nj), rng.uniform(-2, 2, nj)
        x, xR1 = R.line_terms(x0, xg, H)
        want = line_reference(x0, xg, H).reshape(H, 2 * nj)
        assert np.abs(x - want).max() <= 2 * EPS * max(np.abs(x0).max(), np.abs(xg).max())
        assert (x[-1, :nj] == xg).all() and (x[:, nj:] == 0).all() and (xR1 == np.concatenate([x0, np.zeros(nj)])).all()
    dt = 0.5
    for nwp, H in ((2, 1), (2, 7), (3, 4), (5, 8), (12, 5), (9, 33)):
        route = rng.uniform(-2, 2, (nwp, nj))
        x, xR1, seg = R.route_terms(route, nwp, dt, H)
        want = cubic_resample(route.T, dt, H)[:, 1:].T
        bound = EPS * (4 * np.abs(route).max() + 2 * nwp * seg)
        assert (np.abs(x[:, :nj] - want) <= bound).all()
        assert (x[-1, :nj] == route[nwp - 1]).all() and (x[:, nj:] == 0).all() and (xR1[:nj] == route[0]).all()
        for i in range(H):                                                            # a sample on a knot is the knot
            k, num = R.route_position(i + 1, nwp, H)
            if num == 0:
                assert (x[i, :nj] == route[k]).all()
    # (3, 4) puts sample 2 on knot 1, (5, 8) every other sample on a knot, (12, 5) has more waypoints than samples
    assert R.route_position(2, 3, 4) == (1, 0) and R.route_position(4, 5, 8) == (2, 0) and R.route_position(1, 12, 5) == (2, 1)
    assert R.route_position(8, 5, 8) == (3, 8)                                         # the end: tau = 1 in the last segment
    one = rng.uniform(-2, 2, (1, nj))
    x, xR1, _ = R.route_terms(np.vstack([one, np.full((3, nj), np.nan)]), 1, dt, 5)
    assert (x[:, :nj] == one).all() and (x[:, nj:] == 0).all() and (xR1 == np.concatenate([one[0], np.zeros(nj)])).all()


def test_dense_con_matches_the_oracle_at_nonzero_u(O):
    """one shape, u != 0, a moving start: row order, signs and the Diff' Bpos u term against the oracle's get_con"""
    nj, H = 3, 5
    robot, rng = O.robotproperty2("M200i"), np.random.default_rng(7)
    x0 = np.array([0.7825, 0.0284, 0.2172])
    kw = dict(Qp=np.eye(nj), Qv=np.eye(nj), Rblk=np.eye(nj), cR=1.0, lim=np.array([1.0, 0.8, 0.6]), max_input_blk=np.ones(nj), epsilon_O=0.1,
              MAX_O_ITER=3)
    s = O.build_sys_info(robot, nj, H, x0, -x0, O.line_reference(x0, -x0, H), **kw)
    s.xR1 = np.concatenate([x0, rng.uniform(-0.1, 0.1, nj)])
    obs = [dict(l=np.array([[3.7, 8.5, 0.001], [3.7, 8.5, 1.2]]).T, D=0.1, epsilon=0.2),
           dict(l=np.array([[3.5, 8.2, 0.3], [3.9, 8.9, 0.8]]).T, D=0.1, epsilon=0.35)]
    u = rng.uniform(-0.5, 0.5, H * nj)
    x_ = O.rollout(H, nj, robot.delta_t, s.xR1, u)
    A, b, dist, _, grad = O.get_con("M200i", s, obs, x_, u)
    assert np.abs(grad).max() > 1e-3 and np.abs(u).min() > 0
    Ar, br, babs = R.dense_con(dist, grad, [0.2, 0.35], s.lim, None, s.xR1, u, robot.delta_t, H, nj, 2)
    assert Ar.shape == A.shape == (2 * H * (1 + 2 * nj), H * nj)
    assert (np.abs(Ar - A) <= 4 * EPS * np.abs(Ar)).all()
    assert (np.abs(br - b) <= R.gamma(H * nj + 3) * babs).all()
    # with limits: 2 nn more rows, the reference's rows unchanged, infinities kept
    lo, hi = np.array([-np.inf, -1.0, -2.0]), np.array([1.5, 1.0, np.inf])
    Al, bl, _ = R.dense_con(dist, grad, [0.2, 0.35], s.lim, (lo, hi), s.xR1, u, robot.delta_t, H, nj, 2)
    nn, rref = H * nj, A.shape[0]
    assert Al.shape == (rref + 2 * nn, nn) and (Al[:rref] == Ar).all() and (bl[:rref] == br).all()
    _, Baug = double_integrator(H, nj, robot.delta_t)
    Bpos = Baug.reshape(H, 2 * nj, nn)[:, :nj].reshape(nn, nn)
    assert (Al[rref:rref + nn] == Bpos).all() and (Al[rref + nn:] == -Bpos).all()
    pos = (s.Aaug @ s.xR1).reshape(H, 2 * nj)[:, :nj]
    fin = np.isfinite(np.tile(hi, H))
    assert np.abs(bl[rref:rref + nn][fin] - (np.tile(hi, H) - pos.reshape(-1))[fin]).max() <= 4 * EPS * 3
    assert (bl[rref:rref + nn][~fin] == np.inf).all() and (bl[rref + nn:].reshape(H, nj)[:, 0] == np.inf).all()
    assert np.abs(bl[rref + nn:].reshape(H, nj)[:, 1:] - (pos[:, 1:] - lo[1:])).max() <= 4 * EPS * 3


def test_order_keys_and_stable_rank():
    d = np.array([[[0.1, 0.5], [0.04, 0.3]], [[0.2, 0.41], [0.06, 0.4]], [[0.01, 0.39], [0.01, 0.39]]])      # (B=3, H=2, nline=2)
    key = R.order_keys(d, [0.05, 0.4])
    assert key.tolist() == [2, 0, 4] and key.dtype == np.int32                         # 0.4 < 0.4 is not a violation
    assert R.stable_rank(key).tolist() == [2, 0, 1]
    assert R.stable_rank([1, 3, 1, 3, 0, 1]).tolist() == [1, 3, 0, 2, 5, 4]
    assert R.stable_rank([0] * 5).tolist() == [0, 1, 2, 3, 4]
