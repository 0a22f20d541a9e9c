"""Validates the test-side soft-QP reference (tests/soft_reference.py) that tests/test_gpu_soft.py checks the device against,
on linearisations whose hard QP really is infeasible: main_2L's second outer iteration and the second iteration of two
oracle-grown RRT routes (the RRTstar_CFS smoothing stage).  CPU only (oracle + scipy HiGHS)."""
import copy

import numpy as np
import pytest

import soft_reference as S

MUS = (1e4, 1e6, 1e8)


def _main_2l(O):
    P = O.problem_main_2L()
    return P, P.sys_info.xR1, P.sys_info.ff


def _rrt_route(O, seed):
    from oracle import rrt_oracle as R
    from test_rrt import _setup
    robot, obs, x0, goal, rg, rs, ratial = _setup(O)
    r = R.find_route(robot, obs, x0, goal, goal, rg, rs, np.zeros(5), ratial, np.random.default_rng(seed), "RRT")
    assert not r["fail"]
    P = O.problem_RRTstar_CFS(r["route"])
    return P, P.sys_info.xR1, P.sys_info.ff


def _second_qp(O, P, xR1, ff):
    s1 = copy.copy(P.sys_info)
    s1.MAX_O_ITER = 1
    w1 = O.optimizer(P.ROBOT, s1, P.obs, "CFS")
    return S.step_qp(O, P.ROBOT, P.sys_info, P.obs, xR1, ff, w1.u, 2, "CFS")


@pytest.mark.parametrize("case", ["main_2L", "rrt_seed1", "rrt_seed5"])
def test_soft_reference_on_infeasible_linearisations(O, case):
    P, xR1, ff = _main_2l(O) if case == "main_2L" else _rrt_route(O, int(case[-1]))
    q = _second_qp(O, P, xR1, ff)
    _, _, _, st, _ = O.qp_solve(q.G, q.g0, q.A, q.b)
    assert st == 2                                                    # the hard QP is infeasible (oracle)
    tstar = S.least_violation(q.A, q.b, q.col)
    assert tstar > 1e-3
    prev = np.inf
    for mu in MUS:
        u, sl, lam, st, kkt = S.soft_qp(O, q.G, q.g0, q.A, q.b, q.col, mu)
        assert st == 0
        assert kkt[:3].max() <= 1e-9, kkt                              # stationarity, primal, dual
        assert kkt[3] <= (1e-9 if mu <= 1e6 else 1e-6), kkt           # complementarity grows with mu
        assert (sl >= -1e-12).all()
        np.testing.assert_allclose(sl, lam[q.col] / mu, rtol=0, atol=1e-12)   # s = lambda / mu
        assert sl.max() >= tstar - 1e-9                                # never below the least possible violation
        assert sl @ sl <= prev * (1 + 1e-9)                            # |s|^2 is non-increasing in mu (the max slack need not be)
        prev = sl @ sl
