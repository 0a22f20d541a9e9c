"""CPU restatement of the inverse-kinematics contract of include/cfs_hip.h ("inverse kinematics"), TEST INFRASTRUCTURE ONLY.

Written from the header's text alone: pose, residual, analytic Jacobian, the starts from the library's counter-based generator
(tree = restart, counter = joint) in Python integers, steps 1-8 of the iteration, the collision rule, the selection.  The pose comes
from the C oracle's forward kinematics (oracle.arm_pos): a robot copy whose last capsule is [tool, tool + tool_axis] gives the tool
point and, as the difference of that capsule's end points, the tool direction; the capsules of the links before it are replaced by
[t, t + e_z] (t = 0 for a DH link, the link's translation for the two-link arm), which gives the joint axes the Jacobian needs.
Sequential, one restart at a time, plain numpy.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O

MASK = (1 << 64) - 1
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, STEP_CAP = 1e-2, 1e-9, 1e9, 0.5


def uniform(seed, restart, joint):
    """the RRT generator of include/cfs_hip.h with tree = restart, counter = joint"""
    z = (seed + restart * 0x9E3779B97F4A7C15 + (joint + 1) * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def default_tool(robot, nj):
    p = np.asarray(robot.cap[nj - 1], float)
    d = p[:, 1] - p[:, 0]
    n = np.linalg.norm(d)
    return p[:, 0].copy(), (d / n if n > 0 else np.array([0.0, 0.0, 1.0]))


class Arm:
    """pose and Jacobian of one (oracle robot, njoint, tool, tool_axis)"""

    def __init__(self, robot, nj, tool=None, tool_axis=None):
        t0, a0 = default_tool(robot, nj)
        self.nj = nj
        self.tool = t0 if tool is None else np.asarray(tool, float)
        ax = a0 if tool_axis is None else np.asarray(tool_axis, float)
        self.axis = ax / np.linalg.norm(ax)
        self.robot = robot
        probe = SimpleNamespace(**vars(robot))
        ez = np.array([0.0, 0.0, 1.0])
        # translation of link k (0-based): robot.T(:,k+2) in MATLAB's numbering (Lib/2L/CapPos2.m:25); none for a DH link
        self.t = [np.asarray(robot.T, float)[:, k + 1].copy() if robot.name == "2L" else np.zeros(3) for k in range(nj)]
        caps = []
        for i in range(nj - 1):                               # frame of link i carries the axis of joint i + 1
            caps.append(np.stack([self.t[i + 1], self.t[i + 1] + ez], axis=1))
        caps.append(np.stack([self.tool, self.tool + self.axis], axis=1))
        probe.cap = caps + [np.zeros((3, 2))] * (len(robot.cap) - nj)
        self._rb = O.c_robot(probe)
        self._pos = np.zeros(nj * 6)
        self.base = np.asarray(robot.base, float)

    def frames(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        O.lib().orc_arm_pos(C.byref(self._rb), theta.ctypes.data_as(C.c_void_p), C.c_int(self.nj), self._pos.ctypes.data_as(C.c_void_p))
        return self._pos.reshape(self.nj, 2, 3).copy()

    def pose(self, theta):
        f = self.frames(theta)
        return f[-1, 0], f[-1, 1] - f[-1, 0]

    def pose_jac(self, theta):
        """pos, dir, J (6 x nj): column c = [w_c x (pos - q_c); w_c x dir]"""
        f = self.frames(theta)
        p, a = f[-1, 0], f[-1, 1] - f[-1, 0]
        J = np.zeros((6, self.nj))
        for c in range(self.nj):
            if c == 0:
                w, q = np.array([0.0, 0.0, 1.0]), self.t[0] + self.base
            else:
                w, q = f[c - 1, 1] - f[c - 1, 0], f[c - 1, 0]
            J[:3, c], J[3:, c] = np.cross(w, p - q), np.cross(w, a)
        return p, a, J

    def clearance(self, theta, obs, D):
        """min_j (d_j - D_j), d_j = the oracle's dist_arm (near-zero surrogate included); +inf without obstacles"""
        c = math.inf
        for j in range(len(D)):
            d, _ = O.dist_arm(self.robot, np.asarray(theta, float), np.stack([obs[j, :3], obs[j, 3:]], axis=1))
            c = min(c, d - D[j])
        return c


def clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def starts(seed, restarts, theta_ref, lo, hi):
    nj = len(lo)
    out = np.zeros((restarts, nj))
    out[0] = clamp(np.asarray(theta_ref, float), lo, hi)
    for k in range(1, restarts):
        out[k] = clamp(lo + np.array([uniform(seed, k, c) for c in range(nj)]) * (hi - lo), lo, hi)
    return out


def restart(arm, theta0, tp, ta, lo, hi, max_iter, tol_pos, tol_axis):
    """steps 1-8 of the header for one start; returns (theta, state in {0, 1, 3}, it, e_pos, e_axis); collision is the caller's"""
    use_axis = ta is not None
    theta = np.array(theta0, float)

    def resid(th):
        p, a, J = arm.pose_jac(th)
        r = np.concatenate([p - tp, (a - ta) if use_axis else np.zeros(3)])
        if not use_axis:
            J[3:] = 0.0
        return r, J, float(r @ r)
    r, J, F = resid(theta)
    lam, it = LAMBDA0, 0
    while True:
        ep, ea = float(np.linalg.norm(r[:3])), float(np.linalg.norm(r[3:]))
        if not F < math.inf:
            return theta, 3, it, ep, ea
        if ep <= tol_pos and (not use_axis or ea <= tol_axis):
            return theta, 0, it, ep, ea
        if it >= max_iter:
            return theta, 1, it, ep, ea
        A = J.T @ J + lam * np.eye(len(theta))
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return theta, 3, it, ep, ea
        delta = -np.linalg.solve(L.T, np.linalg.solve(L, J.T @ r))
        s = float(np.max(np.abs(delta)))
        if s > STEP_CAP:
            delta = delta * (STEP_CAP / s)
        trial = clamp(theta + delta, lo, hi)
        r2, J2, F2 = resid(trial)
        if F2 < F:
            theta, r, J, F = trial, r2, J2, F2
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = min(lam * 10.0, LAMBDA_MAX)
        it += 1


def solve(arm, target_pos, target_axis, theta_ref, lo, hi, restarts, max_iter, tol_pos, tol_axis, seed, obs=None, D=None, weight=None,
          perturb=0.0):
    """the whole contract for T targets.  perturb: added to every coordinate of every start, then clamped (the sensitivity probe of
    tests/test_ik_reference.py; 0 = the contract)."""
    target_pos = np.atleast_2d(np.asarray(target_pos, float))
    T, nj = target_pos.shape[0], arm.nj
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    obs = np.zeros((0, 6)) if obs is None else np.asarray(obs, float)
    D = np.zeros(0) if D is None else np.asarray(D, float)
    w = np.ones(nj) if weight is None else np.asarray(weight, float)
    theta_ref = np.broadcast_to(np.asarray(theta_ref, float), (T, nj))
    res = SimpleNamespace(theta=np.full((T, nj), np.nan), status=np.zeros(T, int), selected=np.full(T, -1), n_ok=np.zeros(T, int),
                          err_pos=np.full(T, np.nan), err_axis=np.full(T, np.nan), clearance=np.full(T, np.nan),
                          cand_theta=np.zeros((T, restarts, nj)), cand_status=np.zeros((T, restarts), int), cand_iter=np.zeros((T, restarts), int),
                          cand_err_pos=np.zeros((T, restarts)), cand_err_axis=np.zeros((T, restarts)))
    for t in range(T):
        ta = None
        if target_axis is not None:
            ta = np.asarray(target_axis, float).reshape(-1, 3)[t if np.ndim(target_axis) == 2 else 0]
            ta = ta / np.linalg.norm(ta)
        st0 = starts(seed, restarts, theta_ref[t], lo, hi)
        if perturb:
            st0 = clamp(st0 + perturb, lo, hi)
        best, clear_k = (math.inf, -1), {}
        for k in range(restarts):
            th, st, it, ep, ea = restart(arm, st0[k], target_pos[t], ta, lo, hi, max_iter, tol_pos, tol_axis)
            if st == 0:
                clear_k[k] = arm.clearance(th, obs, D)
                if not clear_k[k] >= 0.0:
                    st = 2
            res.cand_theta[t, k], res.cand_status[t, k], res.cand_iter[t, k] = th, st, it
            res.cand_err_pos[t, k], res.cand_err_axis[t, k] = ep, ea
            if st == 0:
                cost = float(np.sum(w * (th - theta_ref[t]) ** 2))
                if cost < best[0]:
                    best = (cost, k)
        ok = res.cand_status[t] == 0
        res.n_ok[t] = int(ok.sum())
        if best[1] >= 0:
            k = best[1]
            res.theta[t], res.selected[t], res.status[t] = res.cand_theta[t, k], k, 0
            res.err_pos[t], res.err_axis[t], res.clearance[t] = res.cand_err_pos[t, k], res.cand_err_axis[t, k], clear_k[k]
        else:
            res.status[t] = 2 if (res.cand_status[t] == 2).any() else 1
    return res


# ---- the parity case shared by tests/test_ik_reference.py (CPU) and tests/test_gpu_ik.py -----------------------------------------
PARITY = dict(robot="M200i", nj=5, T=2, restarts=32, max_iter=100, tol_pos=1e-6, tol_axis=1e-6, seed=6, config_seed=5)
KICK, SENSITIVE = 1e-12, 1e-8     # the perturbation of every start; a restart whose own answer moves by more than SENSITIVE rad is left out


def in_limit_configs(lim, n, seed, shrink=0.8):
    """n seeded random configurations inside the middle `shrink` of the joint ranges"""
    lim = np.asarray(lim, float)
    u = np.random.default_rng(seed).random((n, lim.shape[0]))
    mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), 0.5 * (lim[:, 1] - lim[:, 0]) * shrink
    return mid + (2.0 * u - 1.0) * half


_parity_cache = {}


def parity_case(lim):
    """(arm, inputs, reference result, left-out mask (T, R), movement, theta tolerance) of the axis-mode parity case.
    Left out: restarts whose final reference residual lies within a factor 2 of a tolerance, and restarts whose reference result
    changes state or moves by more than SENSITIVE rad when every start is moved by KICK.  movement: the largest move of the
    others (restarts converged in both runs); tolerance = max(1000 * movement, 1e-10) rad."""
    key = np.asarray(lim, float).tobytes()
    if key in _parity_cache:
        return _parity_cache[key]
    P = PARITY
    lim = np.asarray(lim, float)
    arm = Arm(O.robotproperty2(P["robot"]), P["nj"])
    q = in_limit_configs(lim, P["T"], P["config_seed"])
    tp, ta = np.zeros((P["T"], 3)), np.zeros((P["T"], 3))
    for t in range(P["T"]):
        tp[t], ta[t] = arm.pose(q[t])
    tref = 0.5 * (lim[:, 0] + lim[:, 1])
    kw = dict(restarts=P["restarts"], max_iter=P["max_iter"], tol_pos=P["tol_pos"], tol_axis=P["tol_axis"], seed=P["seed"])
    ref = solve(arm, tp, ta, tref, lim[:, 0], lim[:, 1], **kw)
    per = solve(arm, tp, ta, tref, lim[:, 0], lim[:, 1], perturb=KICK, **kw)
    near = np.zeros_like(ref.cand_status, bool)
    for e, tol in ((ref.cand_err_pos, P["tol_pos"]), (ref.cand_err_axis, P["tol_axis"])):
        near |= (e > tol / 2) & (e < tol * 2)
    move = np.abs(per.cand_theta - ref.cand_theta).max(axis=2)
    both = (ref.cand_status == 0) & (per.cand_status == 0)
    sensitive = (ref.cand_status != per.cand_status) | (both & (move > SENSITIVE))
    out = near | sensitive
    keep = both & ~out
    movement = float(move[keep].max()) if keep.any() else 0.0
    res = (arm, SimpleNamespace(target_pos=tp, target_axis=ta, theta_ref=tref, q=q, **kw), ref, out, movement, max(1000.0 * movement, 1e-10))
    _parity_cache[key] = res
    return res
