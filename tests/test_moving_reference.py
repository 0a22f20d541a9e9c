"""The test-side reference of per-waypoint obstacles (tests/moving_reference.py) against the oracle itself (CPU): with the same
obstacle row at every waypoint it IS O.optimizer, and its per-waypoint distances are O.dist_arm against each waypoint's own row."""
from types import SimpleNamespace

import numpy as np
import pytest

import moving_reference as MR
from motionplanning_5d_m_amd import workloads


def _oracle_dist(O):
    robot = O.robotproperty2("M200i")

    def dist_fn(rb, th, ob):
        return np.array([[O.dist_arm(robot, t, np.stack([o[:3], o[3:]], axis=1))[0] for o in ob] for t in th])
    return dist_fn


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_constant_rows_reproduce_the_oracle_on_main_fanuc(O, mode):
    P = O.problem_main_FANUC()
    s = P.sys_info
    nz = np.random.default_rng(3).normal(0.0, 0.1, (20, s.H * 5)) if mode == "PSGCFS" else None
    want = O.optimizer(P.ROBOT, s, P.obs, mode, noise=nz)
    traj = np.broadcast_to(O.obs_array(P.obs)[None], (s.H, len(P.obs), 6))
    margin = [o["epsilon"] if mode == "CFS" else o["D"] for o in P.obs]
    got = MR.optimizer_moving(O, P.ROBOT, s, traj, margin, mode, s.x_, s.xR1, s.ff, s.caug, noise=nz)
    assert (got.status, got.iter_O, got.total_iter) == (want.status, want.iter_O, want.total_iter)
    assert np.abs(got.x_ - want.x_).max() <= 1e-12
    np.testing.assert_allclose(got.cost_all, want.cost_all, rtol=1e-12)


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_constant_rows_reproduce_the_oracle_on_config3(O, mode):
    s, bt = workloads.config3(_oracle_dist(O), B=3, nobs=8, seed=20260101)
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    want = O.optimizer_batch(O.robotproperty2("M200i"), mode, s.H, 5, bt.x_init, bt.xR1, s.QQ, bt.ff, bt.caug, s.Aaug, s.Baug,
                             s.lim, s.MAX_input, bt.obs, margin, s.epsilon_O, s.MAX_O_ITER, s.alpha,
                             noise=bt.noise if mode == "PSGCFS" else None, nthreads=1)
    for b in range(bt.B):
        traj = np.broadcast_to(bt.obs[b][None], (s.H, bt.nobs, 6))
        got = MR.optimizer_moving(O, "M200i", s, traj, margin, mode, bt.x_init[b], bt.xR1[b], bt.ff[b], bt.caug[b],
                                  noise=bt.noise[b] if mode == "PSGCFS" else None)
        assert (got.status, got.iter_O) == (int(want.status[b]), int(want.iter_O[b])), b
        assert np.abs(got.x_ - want.x_[b]).max() <= 1e-12, b


def test_per_waypoint_distances_are_dist_arm_of_each_waypoints_own_row(O):
    s, bt = workloads.config3_moving(_oracle_dist(O), B=2, nobs=3, seed=11, speed=0.05)
    robot = O.robotproperty2("M200i")
    for b in range(bt.B):
        s3 = SimpleNamespace(**vars(s))
        s3.xR1, s3.robot = bt.xR1[b], robot
        x_ = bt.x_init[b]
        A, rhs, dist, lid, grad = MR.get_con_moving(O, "M200i", s3, bt.obs[b], bt.margin_cfs, x_, np.zeros(s.H * 5), "CFS")
        th = x_.reshape(s.H, 10)[:, :5]
        for i in range(s.H):
            for j in range(bt.nobs):
                d, k = O.dist_arm(robot, th[i], np.stack([bt.obs[b, i, j, :3], bt.obs[b, i, j, 3:]], axis=1))
                assert dist[j, i] == d and lid[j, i] == k
                np.testing.assert_array_equal(grad[j, i], O.num_jac_dist(robot, th[i], np.stack([bt.obs[b, i, j, :3], bt.obs[b, i, j, 3:]], axis=1)))
        assert not np.array_equal(bt.obs[b, 0], bt.obs[b, -1])      # the rows really move
