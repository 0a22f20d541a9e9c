"""Test-side reference of per-waypoint obstacles (include/cfs_hip.h, CFS_OBS_PER_WAYPOINT), built on the
oracle's own primitives.  Collision row (j, i) of get_con (Lib/CFS_FANUC.m:110-120) depends only on waypoint i's pose and on
obstacle j, so the per-waypoint get_con takes, from one oracle get_con per waypoint i (with the obstacles of waypoint i), the rows
of waypoint i.  The outer loop is tests/reference_loop.py's restatement of orc_optimizer (oracle/cfs_oracle.c) on top of it.
Used by tests/test_moving_reference.py (which validates it against O.optimizer) and
tests/test_gpu_moving.py (which checks the device against it)."""
import numpy as np

import reference_loop as RL


def obs_cell(rows, margin):
    """(nobs, 6) rows -> the oracle's obs cell, margin as both epsilon (CFS) and D (PSGCFS)"""
    return [dict(l=np.stack([np.asarray(r[:3], float), np.asarray(r[3:], float)], axis=1), epsilon=float(m), D=float(m))
            for r, m in zip(rows, margin)]


def get_con_moving(O, ROBOT, s, obs_traj, margin, x_, u, mode):
    """get_con with obstacle rows per waypoint.  obs_traj: (H, nobs, 6); s needs xR1.  Returns (Ainq, binq, dist (nobs, H),
    linkid (nobs, H), grad (nobs, H, nj)) in the reference's row order (rows (j*H + i)*(1+2nj) ... belong to (j, i))."""
    H, nj = s.H, s.njoint
    nobs, per = obs_traj.shape[1], 1 + 2 * nj
    A, b = np.zeros((nobs * H * per, H * nj)), np.zeros(nobs * H * per)
    dist, lid, grad = np.zeros((nobs, H)), np.zeros((nobs, H), np.int32), np.zeros((nobs, H, nj))
    for i in range(H):
        Ai, bi, di, li, gi = O.get_con(ROBOT, s, obs_cell(obs_traj[i], margin), x_, u, mode=mode)
        for j in range(nobs):
            r = slice((j * H + i) * per, (j * H + i + 1) * per)
            A[r], b[r] = Ai[r], bi[r]
        dist[:, i], lid[:, i], grad[:, i] = di[:, i], li[:, i], gi[:, i]
    return A, b, dist, lid, grad


def optimizer_moving(O, ROBOT, s, obs_traj, margin, mode, x_init, xR1, ff, caug, noise=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem with obstacle rows per waypoint (reference_loop.optimizer with
    get_con_moving).  obs_traj: (H, nobs, 6); noise: (rows, nn) or None.  Returns a namespace like O.optimizer's (u, x_, iter_O,
    total_iter, status, cost_all, e_cost_all, e_u_all)."""
    return RL.optimizer(O, ROBOT, s, mode, lambda s2, x_, u: get_con_moving(O, ROBOT, s2, obs_traj, margin, x_, u, mode),
                        x_init, xR1, ff, caug, noise=noise)


def batch_moving(O, s, bt, mode, idx, x_init=None, workers=16):
    """optimizer_moving for problems idx of a config3_moving batch"""
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    xi = bt.x_init if x_init is None else x_init

    def one(b):
        nz = bt.noise[b] if (mode == "PSGCFS" and bt.noise is not None) else None
        return optimizer_moving(O, "M200i", s, bt.obs[b], margin, mode, xi[b], bt.xR1[b], bt.ff[b], bt.caug[b], noise=nz)
    return RL.batch(one, idx, workers)


def chaotic_moving(O, s, bt, mode, idx, want, kick=1e-12, move=1e-6, seed=1):
    """reference_loop.chaotic for the moving reference.  Returns (mask, moved_by)."""
    return RL.chaotic(lambda idx_, xi: batch_moving(O, s, bt, mode, idx_, x_init=xi), bt, idx, want, kick, move, seed)
