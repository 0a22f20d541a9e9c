"""CPU restatement of the tool-path contract of include/cfs_hip.h ("Tool paths"), TEST INFRASTRUCTURE ONLY.

Written from the header's text alone: for every candidate the rows of the polyline, `ik_reference.restart` (steps 1-8 of "inverse
kinematics") looped over the N rows from the configuration before each (row 0: from the start), the joint-jump test against that
configuration at every row, `Arm.clearance` for collisions, then the selection on the cost of the START.  Sequential, one candidate
at a time, plain numpy.  The result has the fields of `cart_reference.trace`, so `cart_mesh_reference.apply_meshes` takes it as the
line-only answer.
"""
import math
from types import SimpleNamespace

import numpy as np

import cart_reference as CR
import ik_reference as R
from oracle import oracle as O

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


def candidate(arm, start, state0, pos, axis, lo, hi, K, max_iter, max_joint_step, tol_pos, tol_axis, obs, D):
    """one candidate: (state, done, iterations, end (nj), path (N, nj) with NaN rows after the accepted ones, clearance,
    (e_pos, e_axis) of the last iteration's residual)"""
    nj = arm.nj
    N = (pos.shape[0] - 1) * K + 1
    path = np.full((N, nj), np.nan)
    start = np.asarray(start, float)
    if state0 != 0 or not (np.isfinite(start).all() and (start >= lo).all() and (start <= hi).all()):
        return 5, 0, 0, np.full(nj, np.nan), path, math.inf, (math.nan, math.nan)
    th, clear, its, err = start.copy(), math.inf, 0, (0.0, 0.0)
    for n in range(N):
        done = max(n - 1, 0)
        pn, an = row_pose(pos, axis, n, K)
        if isinstance(an, str):
            return 3, done, its, th, path, clear, err
        new, st, it, ep, ea = R.restart(arm, th, pn, an, lo, hi, max_iter, tol_pos, tol_axis)
        its, err = its + it, (ep, ea)
        if st != 0:
            return st, done, its, new, path, clear, err
        if np.max(np.abs(new - th)) > max_joint_step:
            return 4, done, its, new, path, clear, err
        c = arm.clearance(new, obs, D)
        if not c >= 0.0:
            return 2, done, its, new, path, clear, err
        th, clear = new, min(clear, c)
        path[n] = th
    return 0, N - 1, its, th, path, clear, err


def follow(arm, start, path_pos, path_axis, theta_ref, lo, hi, steps, max_iter, max_joint_step, tol_pos, tol_axis, start_state=None,
           obs=None, D=None, weight=None, perturb=0.0):
    """the whole contract for T targets: path_pos (T, M, 3), path_axis (T, M, 3) or None.  perturb: added to every coordinate of
    every start (the sensitivity probe; 0 = the contract)."""
    start = np.asarray(start, float)
    if start.ndim == 2:
        start = start[None]
    T, Rn, nj = start.shape
    path_pos = np.asarray(path_pos, float).reshape(T, -1, 3)
    M = path_pos.shape[1]
    axes = None if path_axis is None else unit_rows(np.asarray(path_axis, float).reshape(T, M, 3))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    obs = np.zeros((0, 6)) if obs is None else np.asarray(obs, float)
    D = np.zeros(0) if D is None else np.asarray(D, float)
    w = np.ones(nj) if weight is None else np.asarray(weight, float)
    theta_ref = np.broadcast_to(np.asarray(theta_ref, float), (T, nj))
    ss = np.zeros((T, Rn), int) if start_state is None else np.asarray(start_state).reshape(T, Rn)
    N = (M - 1) * steps + 1
    res = SimpleNamespace(theta=np.full((T, nj), np.nan), status=np.zeros(T, int), path=np.full((T, N, nj), np.nan), selected=np.full(T, -1),
                          n_ok=np.zeros(T, int), n_done=np.zeros(T, int), clearance=np.full(T, np.nan), cand_status=np.zeros((T, Rn), int),
                          cand_done=np.zeros((T, Rn), int), cand_iter=np.zeros((T, Rn), int), cand_end=np.zeros((T, Rn, nj)),
                          cand_path=np.zeros((T, Rn, N, nj)), cand_clear=np.zeros((T, Rn)), cand_err=np.zeros((T, Rn, 2)))
    for t in range(T):
        best = (math.inf, -1)
        for r in range(Rn):
            st, done, its, end, path, clear, err = candidate(arm, start[t, r] + perturb, ss[t, r], path_pos[t], None if axes is None else axes[t],
                                                             lo, hi, steps, max_iter, max_joint_step, tol_pos, tol_axis, obs, D)
            res.cand_status[t, r], res.cand_done[t, r], res.cand_iter[t, r] = st, done, its
            res.cand_end[t, r], res.cand_path[t, r], res.cand_clear[t, r], res.cand_err[t, r] = end, path, clear, err
            if st == 0:
                cost = 0.0
                for c in range(nj):
                    dlt = float(start[t, r, c] + perturb) - float(theta_ref[t, c])
                    cost = cost + float(w[c]) * (dlt * dlt)
                if cost < best[0]:
                    best = (cost, r)
        res.n_ok[t] = int((res.cand_status[t] == 0).sum())
        res.n_done[t] = int(res.cand_done[t].max())
        if best[1] >= 0:
            r = best[1]
            res.theta[t], res.selected[t], res.status[t] = start[t, r] + perturb, r, 0
            res.path[t], res.clearance[t] = res.cand_path[t, r], res.cand_clear[t, r]
        else:
            res.status[t] = 1 if (res.cand_status[t] != 5).any() else 2
    return res


# ---- the parity case shared by tests/test_cart_follow_reference.py (CPU) and tests/test_gpu_cart_follow.py -----------------------------
# axis mode on the M200i.  n seeded configurations q; target i's path is P0 = pos(q_i), P1 = P0 + reach*a, P2 = P1 + side*e with
# e = unit(a x z), the axis a of q_i kept on all three poses.  Three candidates per target: q_i (row 0 takes 0 iterations), q_i + 0.02
# (row 0 iterates, inside the jump bound) and q_{i+1} (from elsewhere).  Settings: (reach, side, K).
PARITY = dict(robot="M200i", nj=5, n=24, config_seed=5, shrink=0.6, near=0.02, settings=((0.1, 0.1, 4), (0.2, 0.15, 2)), max_iter=20,
              tol_pos=1e-6, tol_axis=1e-6, max_joint_step=0.3)
KICK = CR.KICK

_parity_cache = {}


def parity_case(lim):
    """(arm, cases, movement, path tolerance); a case per setting holds the inputs, the reference result `ref`, the left-out mask
    `out` (T, R) and its own movement.  Left out, by the two rules of cart_reference.parity_case: candidates whose state or cand_done
    changes when every start is moved by KICK, and candidates whose failing residual (state 1) lies within a factor 2 of a tolerance.
    movement: the largest move of any path configuration of the others; tolerance = max(1000 * movement, 1e-10) rad."""
    key = np.asarray(lim, float).tobytes()
    if key in _parity_cache:
        return _parity_cache[key]
    P = PARITY
    lim = np.asarray(lim, float)
    arm = R.Arm(O.robotproperty2(P["robot"]), P["nj"])
    n = P["n"]
    q = R.in_limit_configs(lim, n, P["config_seed"], shrink=P["shrink"])
    start = np.stack([q, q + P["near"], np.roll(q, -1, axis=0)], axis=1)                       # (n, 3, nj)
    poses = [arm.pose(x) for x in q]
    cases = []
    for reach, side, steps in P["settings"]:
        pos, axs = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
        for i, (p, a) in enumerate(poses):
            e = np.cross(a, [0.0, 0.0, 1.0])
            e = e / np.linalg.norm(e)
            pos[i] = [p, p + reach * a, p + reach * a + side * e]
            axs[i] = a
        kw = dict(steps=steps, max_iter=P["max_iter"], max_joint_step=P["max_joint_step"], tol_pos=P["tol_pos"], tol_axis=P["tol_axis"])
        ref = follow(arm, start, pos, axs, q, lim[:, 0], lim[:, 1], **kw)
        per = follow(arm, start, pos, axs, q, lim[:, 0], lim[:, 1], perturb=KICK, **kw)
        out = (ref.cand_status != per.cand_status) | (ref.cand_done != per.cand_done)
        for col, tol in ((0, P["tol_pos"]), (1, P["tol_axis"])):
            e = ref.cand_err[:, :, col]
            out |= (ref.cand_status == 1) & (e > tol / 2) & (e < tol * 2)
        move = np.nan_to_num(np.abs(per.cand_path - ref.cand_path), nan=0.0).max(axis=(2, 3))
        movement = float(move[~out].max()) if (~out).any() else 0.0
        cases.append(SimpleNamespace(start=start, path_pos=pos, path_axis=axs, theta_ref=q, kw=kw, ref=ref, out=out, movement=movement,
                                     reach=reach, side=side))
    movement = max(c.movement for c in cases)
    res = (arm, cases, movement, max(1000.0 * movement, 1e-10))
    _parity_cache[key] = res
    return res
