"""CPU restatement of the tool-path contract of include/cfs_hip.h ("Tool paths"), TEST INFRASTRUCTURE ONLY.

Written from the header's text alone: for every candidate the rows of the polyline, `ik_reference.restart` (steps 1-8 of "inverse
kinematics") looped over the N rows from the configuration before each (row 0: from the start), the joint-jump test against that
configuration at every row, `Arm.clearance` for collisions, then the selection on the cost of the START.  Sequential, one candidate
at a time, plain numpy.  The loop over the rows, the selection and the parity mask are `cart_reference`'s (`walk`, `select`,
`parity_cases`), with the rows of the polyline below as the poses and row 0 a pose to reach; the result has the fields of
`cart_reference.trace`, so `cart_mesh_reference.apply_meshes` takes it as the line-only answer.
"""
import numpy as np

import cart_reference as CR

AXIS_MIN = CR.AXIS_MIN


def unit_rows(a):
    a = np.asarray(a, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt((a * a).sum(axis=-1, keepdims=True))


def row_pose(pos, axis, n, K):
    """(p_n, a_n) of the header for one target's tables pos (M, 3) and axis (M, 3; rows normalised) or None; a_n is None in
    position-only mode and the string "numeric" when |b| <= 1e-6 or not finite"""
    if n == 0:
        return pos[0], (None if axis is None else axis[0])
    i = (n - 1) // K
    s = (n - i * K) / K
    p = pos[i] + s * (pos[i + 1] - pos[i])
    if axis is None:
        return p, None
    b = (1.0 - s) * axis[i] + s * axis[i + 1]
    nb = float(np.sqrt(b @ b))
    if not nb > AXIS_MIN:
        return p, "numeric"
    return p, b / nb


def rows_of(pos, axis, K):
    """every row of one target's polyline: (N, 3) points and (N, 3) axes (NaN rows where the axis is undefined; None without axes)"""
    M = pos.shape[0]
    N = (M - 1) * K + 1
    pk, ak = np.zeros((N, 3)), (None if axis is None else np.full((N, 3), np.nan))
    for n in range(N):
        p, a = row_pose(pos, axis, n, K)
        pk[n] = p
        if axis is not None and not isinstance(a, str):
            ak[n] = a
    return pk, ak


def _polyline(pos, axis, K):
    """`pose` of one target's polyline: the rows do not depend on the start"""
    return lambda start, n: row_pose(pos, axis, n, K)


def candidate(arm, start, state0, pos, axis, lo, hi, K, max_iter, max_joint_step, tol_pos, tol_axis, obs, D):
    """one candidate of a polyline with K sub-steps per segment: `cart_reference.walk`'s tuple"""
    return CR.walk(arm, start, state0, (pos.shape[0] - 1) * K + 1, _polyline(pos, axis, K), True, lo, hi, max_iter, max_joint_step, tol_pos,
                   tol_axis, obs, D)


def follow(arm, start, path_pos, path_axis, theta_ref, lo, hi, steps, max_iter, max_joint_step, tol_pos, tol_axis, start_state=None,
           obs=None, D=None, weight=None, perturb=0.0):
    """the whole contract for T targets: path_pos (T, M, 3), path_axis (T, M, 3) or None.  perturb: added to every coordinate of
    every start (the sensitivity probe; 0 = the contract)."""
    start = np.asarray(start, float)
    if start.ndim == 2:
        start = start[None]
    T = start.shape[0]
    path_pos = np.asarray(path_pos, float).reshape(T, -1, 3)
    M = path_pos.shape[1]
    axes = None if path_axis is None else unit_rows(np.asarray(path_axis, float).reshape(T, M, 3))
    return CR.select(arm, start, (M - 1) * steps + 1, lambda t: _polyline(path_pos[t], None if axes is None else axes[t], steps), True,
                     theta_ref, lo, hi, max_iter, max_joint_step, tol_pos, tol_axis, start_state, obs, D, weight, perturb)


# ---- the parity case shared by tests/test_cart_follow_reference.py (CPU) and tests/test_gpu_cart_follow.py -----------------------------
# axis mode on the M200i.  n seeded configurations q; target i's path is P0 = pos(q_i), P1 = P0 + reach*a, P2 = P1 + side*e with
# e = unit(a x z), the axis a of q_i kept on all three poses.  Three candidates per target: q_i (row 0 takes 0 iterations), q_i + 0.02
# (row 0 iterates, inside the jump bound) and q_{i+1} (from elsewhere).  Settings: (reach, side, K).
PARITY = dict(robot="M200i", nj=5, n=24, config_seed=5, shrink=0.6, near=0.02, settings=((0.1, 0.1, 4), (0.2, 0.15, 2)), max_iter=20,
              tol_pos=1e-6, tol_axis=1e-6, max_joint_step=0.3)
KICK = CR.KICK


def parity_case(lim):
    """`cart_reference.parity_cases` (its two rules, its movement and tolerance) of the L-shaped paths above"""
    def inputs(arm, q, setting):
        reach, side, steps = setting
        n = q.shape[0]
        pos, axs = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
        for i, (p, a) in enumerate(arm.pose(x) for x in q):
            e = np.cross(a, [0.0, 0.0, 1.0])
            e = e / np.linalg.norm(e)
            pos[i] = [p, p + reach * a, p + reach * a + side * e]
            axs[i] = a
        start = np.stack([q, q + PARITY["near"], np.roll(q, -1, axis=0)], axis=1)              # (n, 3, nj)
        return steps, dict(start=start, path_pos=pos, path_axis=axs, reach=reach, side=side)
    return CR.parity_cases(PARITY, lim, inputs, lambda arm, q, c, lo, hi, **kw: follow(arm, c.start, c.path_pos, c.path_axis, q, lo, hi, **kw))
