"""Test-side reference of joint position limits (include/cfs_hip.h, cfs_problem_set_joint_limits), built on
the oracle's own primitives.  The limited get_con is the oracle's dense get_con (Lib/CFS_FANUC.m:101-135) followed by the position
rows of every waypoint i and joint c: +Bpos row (i, c) <= hi_c - theta0_c - (i+1) dt v0_c, then -Bpos row (i, c) <= theta0_c +
(i+1) dt v0_c - lo_c, with Bpos the position rows of Baug.  The outer loop is tests/reference_loop.py's restatement of
orc_optimizer (oracle/cfs_oracle.c) with these rows appended to every QP; the QP leaves out the rows with an infinite bound: they
can never be active.  Used by tests/test_limits_reference.py (which validates it against
O.optimizer) and tests/test_gpu_limits.py (which checks the device against it)."""
from types import SimpleNamespace

import numpy as np

import reference_loop as RL
from moving_reference import obs_cell


def pos_rows(s, xR1, limits):
    """(A (2nn, nn), b (2nn,)): the position rows [+pos (i, c) | -pos (i, c)] of a limited handle.  limits: (nj, 2) [lo, hi]."""
    H, nj, ns, dt = s.H, s.njoint, 2 * s.njoint, s.robot.delta_t
    lim = np.asarray(limits, float)
    Baug = np.asarray(s.Baug, float)
    Bpos = np.stack([Baug[i * ns + c] for i in range(H) for c in range(nj)])
    xR1 = np.asarray(xR1, float)
    pos = np.array([xR1[c] + ((i + 1) * dt) * xR1[nj + c] for i in range(H) for c in range(nj)])
    lo, hi = np.tile(lim[:, 0], H), np.tile(lim[:, 1], H)
    return np.vstack([Bpos, -Bpos]), np.concatenate([hi - pos, pos - lo])


def get_con_limited(O, ROBOT, s, obs, x_, u, mode, limits):
    """(Ainq, binq) of a limited handle: the oracle's rows in its order, then the position rows.  s needs xR1."""
    A, b, *_ = O.get_con(ROBOT, s, obs, x_, u, mode=mode)
    Ap, bp = pos_rows(s, s.xR1, limits)
    return np.vstack([A, Ap]), np.concatenate([b, bp])


def qp_limited(O, G, g0, A, b):
    """O.qp_solve without the rows whose bound is infinite; lambda is returned on every row (0 on the left-out ones)."""
    keep = np.isfinite(b)
    x, lam_k, it, st, kkt = O.qp_solve(G, g0, A[keep], b[keep])
    lam = np.zeros(b.size)
    lam[keep] = lam_k
    return x, lam, it, st, kkt


def optimizer_limited(O, ROBOT, s, obs, mode, limits, x_init=None, xR1=None, ff=None, caug=None, noise=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem with joint position limits (reference_loop.optimizer with the
    position rows appended and qp_limited).  obs: the oracle's obs cell; limits: (nj, 2); noise: (rows, nn) or None.  Returns a
    namespace like O.optimizer's (u, x_, iter_O, total_iter, status, cost_all, e_cost_all, e_u_all)."""
    x_init = s.x_ if x_init is None else x_init
    xR1 = s.xR1 if xR1 is None else xR1
    ff = s.ff if ff is None else ff
    caug = s.caug if caug is None else caug
    s2 = SimpleNamespace(**vars(s))
    s2.robot = O.robotproperty2(ROBOT)
    return RL.optimizer(O, ROBOT, s, mode, lambda s2_, x_, u: O.get_con(ROBOT, s2_, obs, x_, u, mode=mode), x_init, xR1, ff, caug,
                        noise=noise, extra_rows=pos_rows(s2, xR1, limits), qp=lambda G, g0, A, b: qp_limited(O, G, g0, A, b))


def batch_limited(O, s, bt, mode, idx, limits, x_init=None, workers=16):
    """optimizer_limited for problems idx of a config3 batch"""
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    xi = bt.x_init if x_init is None else x_init

    def one(b):
        nz = bt.noise[b] if (mode == "PSGCFS" and bt.noise is not None) else None
        return optimizer_limited(O, "M200i", s, obs_cell(bt.obs[b], margin), mode, limits, x_init=xi[b], xR1=bt.xR1[b],
                                 ff=bt.ff[b], caug=bt.caug[b], noise=nz)
    return RL.batch(one, idx, workers)


def chaotic_limited(O, s, bt, mode, idx, want, limits, kick=1e-12, move=1e-6, seed=1):
    """reference_loop.chaotic for the limited reference.  Returns (mask, moved_by)."""
    return RL.chaotic(lambda idx_, xi: batch_limited(O, s, bt, mode, idx_, limits, x_init=xi), bt, idx, want, kick, move, seed)
