"""CPU restatement of the Cartesian-path contract of include/cfs_hip.h ("Cartesian paths"), TEST INFRASTRUCTURE ONLY, and the
candidate loop, the selection and the parity-case mask that tests/cart_follow_reference.py ("Tool paths") shares with it.

Written from the header's text alone: for every candidate the line points, `ik_reference.restart` (steps 1-8 of "inverse
kinematics") looped over the steps from theta_{k-1}, the joint-jump test, `Arm.clearance` for collisions, then the selection on the
cost of the START.  Sequential, one candidate at a time, plain numpy.  The two contracts differ in where row n's pose comes from
and in row 0: the line's is the start itself, a tool path's is a pose to reach like every later row.
"""
import math
from types import SimpleNamespace

import numpy as np

import ik_reference as R
from oracle import oracle as O

AXIS_MIN = 1e-6


def line_point(p0, a0, tp, ta, k, K):
    """(p_k, a_k) of the header; a_k is None in position-only mode and the string "numeric" when |b| <= 1e-6"""
    s = k / K
    pk = p0 + s * (tp - p0)
    if ta is None:
        return pk, None
    b = (1.0 - s) * a0 + s * ta
    n = float(np.linalg.norm(b))
    if not n > AXIS_MIN:
        return pk, "numeric"
    return pk, b / n


def walk(arm, start, state0, N, pose, reach_row0, lo, hi, max_iter, max_joint_step, tol_pos, tol_axis, obs, D):
    """one candidate over the N rows of its path: (state, done, iterations, end (nj), path (N, nj) with NaN rows after the accepted
    ones, clearance, (e_pos, e_axis) of the last iteration's residual).  pose(start, n): (p_n, a_n) of row n, a_n None in
    position-only mode and a string where it is undefined.  reach_row0: row 0 is a pose to reach from the start and jump-tested
    against it (a tool path); otherwise it is the start itself and only tested for collision (a line)."""
    nj = arm.nj
    path = np.full((N, nj), np.nan)
    start = np.asarray(start, float)
    if state0 != 0 or not (np.isfinite(start).all() and (start >= lo).all() and (start <= hi).all()):
        return 5, 0, 0, np.full(nj, np.nan), path, math.inf, (math.nan, math.nan)
    th, clear, its, err = start.copy(), math.inf, 0, (0.0, 0.0)
    for n in range(N):
        done, new = max(n - 1, 0), th
        if n or reach_row0:
            pn, an = pose(start, n)
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


def select(arm, start, N, pose_of, reach_row0, theta_ref, lo, hi, max_iter, max_joint_step, tol_pos, tol_axis, start_state, obs, D, weight,
           perturb):
    """the whole contract for T targets with N rows each: `walk` for every candidate (pose_of(t): the `pose` of target t), then the
    selection.  perturb: added to every coordinate of every start (the sensitivity probe; 0 = the contract)."""
    T, Rn, nj = start.shape
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    obs = np.zeros((0, 6)) if obs is None else np.asarray(obs, float)
    D = np.zeros(0) if D is None else np.asarray(D, float)
    w = np.ones(nj) if weight is None else np.asarray(weight, float)
    theta_ref = np.broadcast_to(np.asarray(theta_ref, float), (T, nj))
    ss = np.zeros((T, Rn), int) if start_state is None else np.asarray(start_state).reshape(T, Rn)
    res = SimpleNamespace(theta=np.full((T, nj), np.nan), status=np.zeros(T, int), path=np.full((T, N, nj), np.nan), selected=np.full(T, -1),
                          n_ok=np.zeros(T, int), n_done=np.zeros(T, int), clearance=np.full(T, np.nan), cand_status=np.zeros((T, Rn), int),
                          cand_done=np.zeros((T, Rn), int), cand_iter=np.zeros((T, Rn), int), cand_end=np.zeros((T, Rn, nj)),
                          cand_path=np.zeros((T, Rn, N, nj)), cand_clear=np.zeros((T, Rn)), cand_err=np.zeros((T, Rn, 2)))
    for t in range(T):
        pose, best = pose_of(t), (math.inf, -1)
        for r in range(Rn):
            st, done, its, end, path, clear, err = walk(arm, start[t, r] + perturb, ss[t, r], N, pose, reach_row0, lo, hi, max_iter,
                                                        max_joint_step, tol_pos, tol_axis, obs, D)
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


def _line(arm, tp, ta, K):
    """`pose` of one target's line: from the start's own pose to (tp, ta normalised | None)"""
    return lambda start, k: line_point(*arm.pose(start), tp, ta, k, K)


def candidate(arm, start, state0, tp, ta, lo, hi, K, max_iter, max_joint_step, tol_pos, tol_axis, obs, D):
    """one candidate of a line with K steps: `walk`'s tuple"""
    return walk(arm, start, state0, K + 1, _line(arm, tp, ta, K), False, lo, hi, max_iter, max_joint_step, tol_pos, tol_axis, obs, D)


def trace(arm, start, target_pos, target_axis, theta_ref, lo, hi, steps, max_iter, max_joint_step, tol_pos, tol_axis, start_state=None,
          obs=None, D=None, weight=None, perturb=0.0):
    """the whole contract for T targets.  perturb: added to every coordinate of every start (the sensitivity probe of
    tests/test_cart_reference.py; 0 = the contract)."""
    start = np.asarray(start, float)
    if start.ndim == 2:
        start = start[None]
    target_pos = np.atleast_2d(np.asarray(target_pos, float))

    def pose_of(t):
        ta = None
        if target_axis is not None:
            ta = np.asarray(target_axis, float).reshape(-1, 3)[t if np.ndim(target_axis) == 2 else 0]
            ta = ta / np.linalg.norm(ta)
        return _line(arm, target_pos[t], ta, steps)
    return select(arm, start, steps + 1, pose_of, False, theta_ref, lo, hi, max_iter, max_joint_step, tol_pos, tol_axis, start_state, obs, D,
                  weight, perturb)


# ---- the parity cases shared by the CPU tests (tests/test_cart_reference.py, tests/test_cart_follow_reference.py) and the GPU tests ---
KICK = 1e-12                      # the perturbation of every start

_parity_cache = {}


def parity_cases(P, lim, inputs, run):
    """(arm, cases, movement, path tolerance) of an axis-mode parity case P (a PARITY dict: n seeded configurations q of its robot);
    a case per setting holds the inputs, the reference result `ref`, the left-out mask `out` (T, R) and its own movement.
    inputs(arm, q, setting) -> (steps, the case's input fields); run(arm, q, case, lo, hi, **kw) -> the restatement's result.
    Left out: candidates whose state or cand_done changes when every start is moved by KICK, and candidates whose failing residual
    (state 1) lies within a factor 2 of a tolerance.  movement: the largest move of any path configuration of the others;
    tolerance = max(1000 * movement, 1e-10) rad."""
    key = (P["settings"], np.asarray(lim, float).tobytes())
    if key in _parity_cache:
        return _parity_cache[key]
    lim = np.asarray(lim, float)
    arm = R.Arm(O.robotproperty2(P["robot"]), P["nj"])
    q = R.in_limit_configs(lim, P["n"], P["config_seed"], shrink=P["shrink"])
    cases = []
    for setting in P["settings"]:
        steps, fields = inputs(arm, q, setting)
        kw = dict(steps=steps, max_iter=P["max_iter"], max_joint_step=P["max_joint_step"], tol_pos=P["tol_pos"], tol_axis=P["tol_axis"])
        c = SimpleNamespace(theta_ref=q, kw=kw, **fields)
        ref = run(arm, q, c, lim[:, 0], lim[:, 1], **kw)
        per = run(arm, q, c, lim[:, 0], lim[:, 1], perturb=KICK, **kw)
        out = (ref.cand_status != per.cand_status) | (ref.cand_done != per.cand_done)
        for col, tol in ((0, P["tol_pos"]), (1, P["tol_axis"])):
            e = ref.cand_err[:, :, col]
            out |= (ref.cand_status == 1) & (e > tol / 2) & (e < tol * 2)
        move = np.nan_to_num(np.abs(per.cand_path - ref.cand_path), nan=0.0).max(axis=(2, 3))
        c.ref, c.out, c.movement = ref, out, float(move[~out].max()) if (~out).any() else 0.0
        cases.append(c)
    movement = max(c.movement for c in cases)
    res = (arm, cases, movement, max(1000.0 * movement, 1e-10))
    _parity_cache[key] = res
    return res


# axis mode on the M200i (5 joints, 5 independent equations: isolated solutions).  n seeded configurations; target i is the pose of
# configuration i moved by `reach` metres along its own tool axis, the axis kept.  Target i has R candidates: configuration i itself
# (an approach of `reach` metres along the tool axis) and its R - 1 successors in the list (long lines from elsewhere, which end in
# joint jumps and steps that do not converge).  Two settings: (reach, steps).
PARITY = dict(robot="M200i", nj=5, n=24, R=3, config_seed=5, shrink=0.6, settings=((0.1, 16), (0.3, 4)), max_iter=20, tol_pos=1e-6,
              tol_axis=1e-6, max_joint_step=0.3)


def parity_case(lim):
    """`parity_cases` of the line: the case of tests/test_cart_reference.py (CPU) and tests/test_gpu_cart.py"""
    def inputs(arm, q, setting):
        reach, steps = setting
        n = q.shape[0]
        poses = [arm.pose(x) for x in q]
        start = np.stack([q[(np.arange(n) + r) % n] for r in range(PARITY["R"])], axis=1)    # (n, R, nj)
        return steps, dict(start=start, target_pos=np.array([p + reach * a for p, a in poses]), target_axis=np.array([a for _, a in poses]),
                           reach=reach)
    return parity_cases(PARITY, lim, inputs, lambda arm, q, c, lo, hi, **kw: trace(arm, c.start, c.target_pos, c.target_axis, q, lo, hi, **kw))
