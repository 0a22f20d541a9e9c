"""Host-side mirror of the reference's solver classes over the C ABI.

``CFS_FANUC(obs, sys_info, ROBOT).optimizer()`` and ``PSGCFS_FANUC(obs, sys_info, ROBOT).optimizer()``
keep the reference's names, argument meaning and result fields (Lib/CFS_FANUC.m:40-79,
Lib/PSGCFS_FANUC.m:43-82, Lib/EVAL.m): ``u, x_, Ainq, binq, iter_O, total_iter, eval.cost_all,
eval.e_cost_all, eval.e_u_all, eval.cost_new``.  Every numerical step happens in libcfs_hip.so on
the GPU; this module only packs arguments.  ``CFSBatch`` is the batched form (the build's added
outer dimension: stochastic seeds, RRT node pairs, start/goal/obstacle variations).
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import _args, _lib
from ._args import f64 as _f64, obs_meshes, ptr as _ptr  # noqa: F401  (other modules and tests import them from here)
from .robotproperty2 import to_c_robot

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def obs_to_array(obs):
    """obs cell -> (nobs, 6) rows [obs{j}.l(:,1); obs{j}.l(:,2)]; mesh obstacles (obs{j}.mesh) get a row of zeros."""
    return _f64(np.stack([np.zeros(6) if "mesh" in o else
                          np.concatenate([np.asarray(o["l"], float)[:, 0], np.asarray(o["l"], float)[:, 1]]) for o in obs]))


def obs_moving(obs):
    """Does any line obstacle of the obs cell move, i.e. is its obs{j}.l 3x2xH (shape (3, 2, H)) instead of 3x2?"""
    return any("mesh" not in o and np.ndim(o["l"]) == 3 for o in obs)


def obs_traj_to_array(obs, H):
    """obs cell -> (H, nobs, 6): row [i][j] = [l(:,1); l(:,2)] of obstacle j at waypoint i+1.  obs{j}.l may be 3x2xH (MATLAB's
    layout: shape (3, 2, H), page i = waypoint i+1) or 3x2, which is broadcast over the horizon (CFS_OBS_PER_WAYPOINT)."""
    H = int(H)
    out = np.zeros((H, len(obs), 6))
    for j, o in enumerate(obs):
        if "mesh" in o:
            raise ValueError("mesh obstacles are static: they cannot be given per waypoint")
        l = np.asarray(o["l"], float)
        if l.shape == (3, 2):
            l = np.broadcast_to(l[:, :, None], (3, 2, H))
        elif l.shape != (3, 2, H):
            raise ValueError(f"obs[{j}]['l'] has shape {l.shape}: expected (3, 2) or (3, 2, H={H})")
        out[:, j, :3], out[:, j, 3:] = l[:, 0, :].T, l[:, 1, :].T
    return _f64(out)


def mesh_pose_array(pose, H):
    """A mesh's rigid poses -> (H, 12): row i = the row-major 3x4 [R | t] that places the mesh in the world at waypoint i+1
    (cfs_problem_set_mesh_motion).  pose: (H, 4, 4) or (H, 3, 4), or one (4, 4) / (3, 4) held over the horizon.  ValueError for any
    other shape, a last row that is not [0, 0, 0, 1], a value that is not finite, and a pose that is not a rigid motion by the
    library's own rule (max|RR' - I| > 1e-9 or det R <= 0: scaled, sheared or mirrored)."""
    H = int(H)
    try:
        T = np.array(pose, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"a mesh pose must be an array of 3x4 or 4x4 matrices, not {pose!r}") from None
    if T.shape in ((4, 4), (3, 4)):
        T = np.broadcast_to(T, (H,) + T.shape)
    if T.shape not in ((H, 4, 4), (H, 3, 4)):
        raise ValueError(f"a mesh pose has shape {T.shape}: expected (H, 4, 4), (H, 3, 4), (4, 4) or (3, 4) with H={H}")
    if not np.isfinite(T).all():
        raise ValueError("a mesh pose holds a value that is not finite")
    if T.shape[1] == 4 and not (T[:, 3, :] == np.array([0.0, 0.0, 0.0, 1.0])).all():
        raise ValueError("the last row of a 4x4 mesh pose must be [0, 0, 0, 1]")
    R = T[:, :3, :3]
    dev = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2))
    det = np.linalg.det(R)
    bad = np.nonzero((dev > 1e-9) | ~(det > 0.0))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"the mesh pose at waypoint {i + 1} is not a rigid motion: max|RR' - I| = {dev[i]:.3g}, det R = {det[i]:.3g}")
    return _f64(T[:, :3, :].reshape(H, 12))


def obs_mesh_poses(obs, H):
    """None when no mesh entry of the obs cell carries a pose, else (nmesh, H, 12): mesh_pose_array of every mesh entry in cell
    order, the identity for an entry without one (it is held still)."""
    entries = [o for o in obs if "mesh" in o]
    if not any("pose" in o for o in entries):
        return None
    return _f64(np.stack([mesh_pose_array(o["pose"] if "pose" in o else np.eye(4), H) for o in entries]))


def _joint_limits_array(joint_limits, robot, nj):
    """None | (nj, 2) float64 [lo, hi] from CFSBatch's joint_limits=: None (no position rows), "robot" (robot.thetamax[:nj]) or an
    (nj, 2) array.  ValueError for anything malformed (wrong shape, NaN, lo >= hi), before the device is touched."""
    if joint_limits is None:
        return None
    if isinstance(joint_limits, str):
        if joint_limits != "robot":
            raise ValueError(f'joint_limits must be None, "robot" or an (njoint, 2) array, not {joint_limits!r}')
        tm = getattr(robot, "thetamax", None)
        if tm is None:
            raise ValueError('joint_limits="robot" needs sys_info.robot.thetamax')
        joint_limits = np.asarray(tm, dtype=np.float64)[:nj]
    try:
        a = np.array(joint_limits, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"joint_limits must be an (njoint, 2) array of [lo, hi], not {joint_limits!r}") from None
    if a.shape != (nj, 2):
        raise ValueError(f"joint_limits has shape {a.shape}: it must be (njoint, 2) = {(nj, 2)}")
    if np.isnan(a).any():
        raise ValueError("joint_limits holds NaN")
    if not (a[:, 0] < a[:, 1]).all():
        raise ValueError(f"joint_limits needs lo < hi on every joint: {a.tolist()}")
    return np.ascontiguousarray(a)


def _infeasible_args(on_infeasible, soft_weight):
    """(policy code, weight) for cfs_problem_set_infeasible_policy; ValueError for anything malformed.  "soften" needs a finite
    soft_weight > 0; "stop" ignores a (valid) weight and passes 1.0 when there is none."""
    policy = _args.code(_lib.INFEASIBLE, on_infeasible, "on_infeasible")
    if soft_weight is None:
        if on_infeasible == "soften":
            raise ValueError('on_infeasible="soften" needs soft_weight= (cost units per m^2 of slack, finite and > 0)')
        return policy, 1.0
    if isinstance(soft_weight, bool) or not isinstance(soft_weight, (int, float, np.integer, np.floating)):
        raise ValueError(f"soft_weight must be a real number, not {soft_weight!r}")
    w = float(soft_weight)
    if not (math.isfinite(w) and w > 0.0):
        raise ValueError(f"soft_weight must be finite and > 0, not {soft_weight!r}")
    return policy, w


# cfs_batch_out: field -> (the handle's attribute that holds its row length, None for one entry per problem; dtype)
SOLVE_OUT = dict(u=("nn", np.float64), x_=("nx", np.float64), cost_all=("K", np.float64), e_cost_all=("K", np.float64),
                 e_u_all=("K", np.float64), iter_O=(None, np.int32), total_iter=(None, np.int32), status=(None, np.int32))
# the (B, nobs) outputs of the clearance audits in argument order; tri_path is cfs_clearance_mesh*'s alone
AUDIT_OUT = dict(dist_wp=np.float64, dist_path=np.float64, dist_lower=np.float64, t_path=np.float64, link_path=np.int32,
                 tri_path=np.int32)


def _batch_in(B, x_init, xR1, ff, caug, obs, noise=None):
    """cfs_batch_in over host arrays or CUDA tensors"""
    return _lib.cfs_batch_in(B=B, x_init=_ptr(x_init), xR1=_ptr(xR1), ff=_ptr(ff), caug=_ptr(caug), obs=_ptr(obs), noise=_ptr(noise),
                             noise_rows=0 if noise is None else noise.shape[1])


class CFSBatch:
    """A problem family (robot, horizon, cost matrix, limits, obstacle count and margins) on one GPU,
    solving batches of problems that differ in start/goal (x_init, xR1, ff, caug), obstacles and noise."""

    def __init__(self, sys_info, nobs, margin, mode="CFS", max_batch=1, device=None, check_dynamics=True, use_weights="auto",
                 jacobian="fd_literal", on_infeasible="stop", soft_weight=None, obstacles="static", joint_limits=None):
        """joint_limits: None (the default: no position rows) | "robot" (sys_info.robot.thetamax[:njoint]) | an (njoint, 2) array of
        [lo, hi] in rad, either side possibly infinite: every QP keeps each waypoint's x_ inside (include/cfs_hip.h,
        cfs_problem_set_joint_limits); get_con then has 2*H*njoint more rows and qp's lambda 2*nn more entries.
        obstacles: "static" (the default: obs arrays are (B, nobs, 6)) | "per_waypoint" (obs arrays of solve, solve_device,
        linearize and get_con are (B, H, nobs, 6), row [b, i, j] = obstacle j at waypoint i+1; no meshes, no chomp;
        include/cfs_hip.h, cfs_problem_set_obstacle_motion).
        on_infeasible: "stop" (the default: a proven-infeasible linearised QP ends the problem with QP_INFEASIBLE) | "soften"
        (that outer iteration solves the soft-constraint QP with weight soft_weight instead and carries on; include/cfs_hip.h,
        cfs_problem_set_infeasible_policy).  Results of solve() carry viol_all (B x MAX_O_ITER) and n_soft (B).
        jacobian: "fd_literal" (num_jac.m literally, the default) | "analytic" (the exact derivative of the active branch of
        dist_arm; include/cfs_hip.h, cfs_problem_set_jacobian).
        use_weights: True -> cfs_problem_create_from_weights(sys_info.weights) (the library assembles QQ, Qaug and alpha
        itself: neither crosses the boundary); False -> cfs_problem_create(sys_info.QQ, ...); "auto" -> the weights path, but
        only if the QQ the library assembles from sys_info.weights IS sys_info.QQ (to 1e-12 of its largest entry; checked
        with cfs_problem_family) and alpha agrees; a sys_info whose QQ / Baug were edited after build_sys_info is solved
        through the dense path with the dynamics check, exactly as given."""
        s = sys_info
        _args.code(_lib.JACOBIAN, jacobian, "jacobian")  # validated before anything touches the device
        _infeasible_args(on_infeasible, soft_weight)
        _args.code(_lib.OBSTACLES, obstacles, "obstacles")
        jl = _joint_limits_array(joint_limits, s.robot, int(s.njoint))
        self.mode = mode
        self.H, self.nj = int(s.H), int(s.njoint)
        self.ns, self.nn, self.nx = 2 * self.nj, self.H * self.nj, self.H * 2 * self.nj
        self.nobs, self.K = int(nobs), int(s.MAX_O_ITER)
        self.max_batch = int(max_batch)
        self.robot = s.robot
        self.rows = self.nobs * self.H * (1 + 2 * self.nj)
        lib = _lib.lib()
        if device is not None:
            _lib.check(lib.cfs_set_device(int(device)))
        d = _lib.cfs_problem_desc()
        d.robot = to_c_robot(s.robot)
        d.mode = _lib.MODE[mode]
        d.H, d.njoint, d.nobs = self.H, self.nj, self.nobs
        wts = getattr(s, "weights", None)
        self.from_weights = bool(use_weights) and wts is not None if use_weights == "auto" else bool(use_weights)
        if use_weights == "auto" and self.from_weights and not self._double_integrator(s):
            self.from_weights = False                    # edited Aaug / Baug: the dense path validates them (CFS_ERR_DYNAMICS)
        if self.from_weights and wts is None:
            raise ValueError("use_weights=True needs sys_info.weights")
        keep = [None if self.from_weights else np.asfortranarray(s.QQ, dtype=np.float64), _f64(s.lim),
                _f64(np.asarray(margin, float).reshape(-1))]
        d.QQ, d.lim, d.margin = _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2])
        if keep[2].size != self.nobs:
            raise ValueError("margin must have one entry per obstacle")
        self.margin = keep[2].copy()
        check_dynamics_asked = check_dynamics
        if self.from_weights:
            check_dynamics = False                       # Aaug / Baug are implied (and built) by the library
        if check_dynamics and getattr(s, "Aaug", None) is not None:
            keep.append(np.asfortranarray(s.Aaug, dtype=np.float64))
            d.Aaug = _ptr(keep[-1])
        if check_dynamics and getattr(s, "Baug", None) is not None:
            keep.append(np.asfortranarray(s.Baug, dtype=np.float64))
            d.Baug = _ptr(keep[-1])
        if mode == "CFS":
            keep.append(_f64(s.MAX_input))
            d.MAX_input = _ptr(keep[-1])
        d.epsilon_O, d.MAX_O_ITER, d.alpha = float(s.epsilon_O), self.K, float(getattr(s, "alpha", 0.0))
        d.max_batch = self.max_batch
        h = C.c_void_p()
        self._lib = lib
        if self.from_weights:
            w = _lib.cfs_cost_weights()
            keep += [np.asfortranarray(wts["Qp"], dtype=np.float64), np.asfortranarray(wts["Qv"], dtype=np.float64),
                     np.asfortranarray(wts["Rblk"], dtype=np.float64)]
            w.Qp, w.Qv, w.Rblk = _ptr(keep[-3]), _ptr(keep[-2]), _ptr(keep[-1])
            w.q_cross, w.w_stage, w.w_terminal, w.cR = float(wts["q_cross"]), float(wts["w_stage"]), float(wts["w_terminal"]), float(wts["cR"])
            _lib.check(lib.cfs_problem_create_from_weights(C.byref(d), C.byref(w), C.byref(h)))
            self._h = h
            if use_weights == "auto" and not self._weights_match(s):
                # the caller's matrices are not the ones its weights assemble: solve what was given, through the dense path
                self.close()
                CFSBatch.__init__(self, sys_info, nobs, margin, mode=mode, max_batch=max_batch, device=device,
                                  check_dynamics=check_dynamics_asked, use_weights=False, jacobian=jacobian,
                                  on_infeasible=on_infeasible, soft_weight=soft_weight, obstacles=obstacles,
                                  joint_limits=joint_limits)
                return
        else:
            _lib.check(lib.cfs_problem_create(C.byref(d), C.byref(h)))
            self._h = h
        if jacobian != "fd_literal":
            self.set_jacobian(jacobian)
        if on_infeasible != "stop":
            self.set_infeasible_policy(on_infeasible, soft_weight)
        if obstacles != "static":
            self.set_obstacle_motion(obstacles)
        if jl is not None:
            self.set_joint_limits(jl)

    def set_joint_limits(self, joint_limits):
        """joint position limits of the following solves and pieces: None (clear) | "robot" | an (njoint, 2) array of [lo, hi]
        (cfs_problem_set_joint_limits)."""
        jl = _joint_limits_array(joint_limits, self.robot, self.nj)
        if jl is None:
            _lib.check(self._lib.cfs_problem_set_joint_limits(self._h, None, None))
        else:
            lo, hi = np.ascontiguousarray(jl[:, 0]), np.ascontiguousarray(jl[:, 1])
            _lib.check(self._lib.cfs_problem_set_joint_limits(self._h, _ptr(lo), _ptr(hi)))
        self.rows = self.nobs * self.H * (1 + 2 * self.nj) + (0 if jl is None else 2 * self.nn)

    def joint_limits(self):
        """(njoint, 2) array of [lo, hi] as set, or None without limits (cfs_problem_get_joint_limits)."""
        on, lo, hi = C.c_int(0), np.zeros(self.nj), np.zeros(self.nj)
        _lib.check(self._lib.cfs_problem_get_joint_limits(self._h, C.byref(on), _ptr(lo), _ptr(hi)))
        return np.stack([lo, hi], axis=1) if on.value else None

    def set_obstacle_motion(self, obstacles):
        """obstacles of the following solves and pieces: "static" | "per_waypoint" (cfs_problem_set_obstacle_motion)."""
        _lib.check(self._lib.cfs_problem_set_obstacle_motion(self._h, _args.code(_lib.OBSTACLES, obstacles, "obstacles")))

    @property
    def obstacle_motion(self):
        m = C.c_int(0)
        _lib.check(self._lib.cfs_problem_get_obstacle_motion(self._h, C.byref(m)))
        return _args.name_of(_lib.OBSTACLES, m.value)

    def _check_obs(self, obs, B):
        """obs must be (B, nobs, 6) on a static handle (assert, as ever) and (B, H, nobs, 6) on a per-waypoint one (ValueError)."""
        if self.obstacle_motion == "per_waypoint":
            if tuple(obs.shape) != (B, self.H, self.nobs, 6):
                raise ValueError(f"obs has shape {tuple(obs.shape)}: a per-waypoint handle takes (B, H, nobs, 6) = {(B, self.H, self.nobs, 6)}")
        else:
            assert tuple(obs.shape) == (B, self.nobs, 6)

    def set_infeasible_policy(self, on_infeasible, soft_weight=None):
        """what the following solves and pieces do with a proven-infeasible QP: "stop" | "soften" (with soft_weight > 0)."""
        code, w = _infeasible_args(on_infeasible, soft_weight)
        _lib.check(self._lib.cfs_problem_set_infeasible_policy(self._h, code, w))

    @property
    def infeasible_policy(self):
        """(policy, soft_weight) as last set; the weight is None under "stop"."""
        m, w = C.c_int(0), C.c_double(0.0)
        _lib.check(self._lib.cfs_problem_get_infeasible_policy(self._h, C.byref(m), C.byref(w)))
        name = _args.name_of(_lib.INFEASIBLE, m.value)
        return name, (w.value if name == "soften" else None)

    def soft_results(self, B):
        """(viol_all (B, MAX_O_ITER), n_soft (B,)) of the last whole solve (synchronises; cfs_soft_results)."""
        viol, ns = np.zeros((B, self.K)), np.zeros(B, np.int32)
        _lib.check(self._lib.cfs_soft_results(self._h, B, _ptr(viol), _ptr(ns)))
        return viol, ns

    def set_jacobian(self, jacobian):
        """linearisation of the line obstacles for the following solves and pieces: "fd_literal" | "analytic"."""
        _lib.check(self._lib.cfs_problem_set_jacobian(self._h, _args.code(_lib.JACOBIAN, jacobian, "jacobian")))

    @property
    def jacobian(self):
        m = C.c_int(0)
        _lib.check(self._lib.cfs_problem_get_jacobian(self._h, C.byref(m)))
        return _args.name_of(_lib.JACOBIAN, m.value)

    def _weights_match(self, s):
        """does the QQ (and alpha) the library assembled from sys_info.weights equal what sys_info carries?"""
        QQ = getattr(s, "QQ", None)
        if QQ is None:
            return True
        QQ = np.asarray(QQ, float)
        got, alpha = self.family()
        if QQ.shape != got.shape or not np.abs(got - QQ).max() <= 1e-12 * np.abs(QQ).max():
            return False
        a = float(getattr(s, "alpha", 0.0))
        return not (self.mode == "PSGCFS" and a != 0.0 and not abs(alpha - a) <= 1e-9 * abs(a))

    def _double_integrator(self, s):
        """is sys_info.Baug (when present) the double integrator the structured products assume (robotproperty2.m:136-139)?"""
        Bm = getattr(s, "Baug", None)
        if Bm is None:
            return True
        dt, H, nj = float(s.robot.delta_t), self.H, self.nj
        Bm = np.asarray(Bm, float)
        if Bm.shape != (H * 2 * nj, H * nj):
            return False
        Bm = Bm.reshape(H, 2 * nj, H, nj)
        i, k = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
        want = np.zeros_like(Bm)
        for c in range(nj):
            want[:, c, :, c] = np.where(k <= i, ((i - k) + 0.5) * dt * dt, 0.0)
            want[:, nj + c, :, c] = np.where(k <= i, dt, 0.0)
        return bool(np.abs(Bm - want).max() <= 1e-12 * (1.0 + np.abs(want).max()))

    def set_launch_order(self, order="auto"):
        """Workgroup w of the next solves handles problem order[w] (cfs_set_launch_order): "auto" (default: most violated
        initial trajectories first), "identity", or a permutation of 0..B-1.  Results do not depend on it; a launch is as
        long as its longest problem plus that problem's wait for a compute unit."""
        if isinstance(order, str):
            _lib.check(self._lib.cfs_set_launch_order(self._h, None, {"auto": 0, "identity": -1}[order]))
            return
        o = np.ascontiguousarray(order, dtype=np.int32)
        _lib.check(self._lib.cfs_set_launch_order(self._h, _ptr(o), int(o.size)))

    def family(self):
        """(QQ, alpha) the handle was built with (cfs_problem_family)."""
        QQ = np.zeros((self.nn, self.nn), order="F")
        a = C.c_double(0.0)
        _lib.check(self._lib.cfs_problem_family(self._h, _ptr(QQ), C.byref(a)))
        return QQ, a.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cfs_problem_destroy(self._h)
            self._h = None

    __del__ = close

    def set_meshes(self, meshes):
        """The last len(meshes) of the nobs obstacles are these mesh.Mesh objects from now on (cfs_problem_set_meshes)."""
        if len(meshes) and self.obstacle_motion == "per_waypoint":
            raise ValueError("mesh obstacles are static: not supported on a per-waypoint handle")
        self._meshes = list(meshes)                      # keep them alive as long as the handle uses them
        self._mesh_motion = False                        # cfs_problem_set_meshes resets the handle to static meshes
        _lib.check(self._lib.cfs_problem_set_meshes(self._h, *_args.mesh_table(self._meshes)[:2]))

    def set_mesh_motion(self, poses):
        """A rigid pose per waypoint for every mesh of the handle (cfs_problem_set_mesh_motion, include/cfs_hip.h): poses is
        (nmesh, H, 12), (nmesh, H, 3, 4) or (nmesh, H, 4, 4), or a sequence of nmesh entries that mesh_pose_array accepts;
        entry [j][i] places mesh j in the world at waypoint i+1.  None: the meshes are static again.  The poses belong to the
        handle and are shared by every problem of a batch."""
        meshes = getattr(self, "_meshes", None)
        if not meshes:
            raise ValueError("set_mesh_motion needs a handle with mesh obstacles (set_meshes)")
        if poses is None:
            _lib.check(self._lib.cfs_problem_set_mesh_motion(self._h, None))
            self._mesh_motion = False
            return
        if len(poses) != len(meshes):
            raise ValueError(f"set_mesh_motion needs one pose sequence per mesh: {len(meshes)}, not {len(poses)}")
        arr = _f64(np.stack([mesh_pose_array(np.asarray(p, float).reshape(self.H, 3, 4) if np.shape(p) == (self.H, 12) else p, self.H)
                             for p in poses]))
        _lib.check(self._lib.cfs_problem_set_mesh_motion(self._h, _ptr(arr)))
        self._mesh_motion = True

    # ---- whole solve ------------------------------------------------------------------------------
    def _outputs(self, B, device=None):
        """the cfs_batch_out namespace for B problems: numpy arrays, or torch tensors on `device`"""
        z = _args.zeros_on(device)
        return SimpleNamespace(**{k: z((B,) if n is None else (B, getattr(self, n)), dt) for k, (n, dt) in SOLVE_OUT.items()})

    def solve(self, x_init, xR1, ff, caug, obs, noise=None):
        """Host arrays in, host arrays out (cfs_solve_batch)."""
        x_init, xR1, ff, caug, obs = _f64(x_init), _f64(xR1), _f64(ff), _f64(caug).reshape(-1), _f64(obs)
        B = x_init.shape[0]
        assert x_init.shape == (B, self.nx) and xR1.shape == (B, self.ns) and ff.shape == (B, self.nn)
        assert caug.shape == (B,)
        self._check_obs(obs, B)
        if noise is not None:
            noise = _f64(noise)
            assert noise.ndim == 3 and noise.shape[0] == B and noise.shape[2] == self.nn
        r = self._outputs(B)
        i, o = _batch_in(B, x_init, xR1, ff, caug, obs, noise), _args.fill(_lib.cfs_batch_out(), r)
        _lib.check(self._lib.cfs_solve_batch(self._h, C.byref(i), C.byref(o)))
        r.viol_all, r.n_soft = self.soft_results(B)
        return r

    def alloc_outputs(self, B, device):
        """Device-resident output buffers (torch CUDA tensors) for solve_device."""
        return self._outputs(B, device)

    def solve_device(self, x_init, xR1, ff, caug, obs, noise=None, out=None, stream=None):
        """torch CUDA tensors in/out; enqueues on `stream` (default: torch's current stream) and
        returns without synchronising (cfs_solve_batch_device)."""
        B = x_init.shape[0]
        for t in (x_init, xR1, ff, caug, obs) + ((noise,) if noise is not None else ()):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        self._check_obs(obs, B)
        if out is None:
            out = self.alloc_outputs(B, x_init.device)
        i, o = _batch_in(B, x_init, xR1, ff, caug, obs, noise), _args.fill(_lib.cfs_batch_out(), out)
        stream = _args.stream_ptr(stream, x_init.device)
        _lib.check(self._lib.cfs_solve_batch_device(self._h, C.byref(i), C.byref(o), C.c_void_p(stream)))
        return out

    # ---- clearance audit between the waypoints, against line obstacles or with mesh obstacles -------------------------
    def _audit(self, mesh, device, x_, u, xR1, obs, substeps, out=None, stream=None, motion=False):
        """the six audit entries: cfs_clearance[_mesh[_motion]][_device].  The line audit takes the obs shape of the handle's
        obstacle motion (_check_obs); the mesh audits take (B, nobs, 6) and never ask the handle.  motion: the entry that admits
        a handle with mesh motion (set_mesh_motion)."""
        S = _args.int_in(substeps, "substeps", 1, 64)
        if mesh and not getattr(self, "_meshes", None):
            raise ValueError(f"clearance_mesh{'_motion' if motion else ''} needs a handle with mesh obstacles (set_meshes): "
                             "use clearance for line obstacles")
        if not mesh and getattr(self, "_meshes", None):
            raise ValueError("the clearance audit measures line obstacles only: this handle has mesh obstacles")
        if mesh and not motion and getattr(self, "_mesh_motion", False):
            raise ValueError("clearance_mesh audits static meshes (its bound takes v_obs = 0): this handle has mesh motion")
        if device:
            B = x_.shape[0]
            for t in (x_, u, xR1, obs):
                assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        else:
            x_, u, xR1, obs = _f64(x_), _f64(u), _f64(xR1), _f64(obs)
            B = x_.shape[0]
        want = [(B, self.nx), (B, self.nn), (B, self.ns)] + ([(B, self.nobs, 6)] if mesh else [])
        got = [tuple(t.shape) for t in (x_, u, xR1, obs)[:len(want)]]
        if got != want:
            raise ValueError(f"x_, u, xR1{', obs' if mesh else ''} must have shapes {want}, not {got}")
        if not mesh:
            self._check_obs(obs, B)
        names = [k for k in AUDIT_OUT if mesh or k != "tri_path"]
        if not device:
            out = SimpleNamespace(**{k: np.zeros((B, self.nobs), AUDIT_OUT[k]) for k in names})
        elif out is None:
            out = (self.alloc_clearance_mesh if mesh else self.alloc_clearance)(B, x_.device)
        args = [self._h, B, S, _ptr(x_), _ptr(u), _ptr(xR1), _ptr(obs)] + [_ptr(getattr(out, k)) for k in names]
        entry = ("cfs_clearance_mesh_motion" if motion else "cfs_clearance_mesh") if mesh else "cfs_clearance"
        if not device:
            _lib.check(getattr(self._lib, entry)(*args))
            out.short_by = (self.margin[None, :] - out.dist_path).max(axis=1)
            return out
        for k in names:
            t = getattr(out, k)
            assert t.is_cuda and t.dtype == getattr(torch, np.dtype(AUDIT_OUT[k]).name) and t.is_contiguous() and tuple(t.shape) == (B, self.nobs)
        cur = torch.cuda.current_stream(x_.device)
        sp = cur.cuda_stream if stream is None else int(stream)
        _lib.check(getattr(self._lib, entry + "_device")(*args, C.c_void_p(sp)))
        if sp == cur.cuda_stream:
            ts = cur
        else:                            # pointer 0 is the default stream: ExternalStream does not wrap it
            ts = torch.cuda.default_stream(x_.device) if sp == 0 else torch.cuda.ExternalStream(sp, device=x_.device)
        with torch.cuda.stream(ts):      # short_by on the same stream, after the audit
            out.short_by = (self._margin_on(x_.device)[None, :] - out.dist_path).amax(dim=1)
        return out

    def clearance(self, x_, u, xR1, obs, substeps=16):
        """Clearance of B trajectories (x_, u as a solve returns them; xR1, obs as given to it) along the motion between the
        waypoints, `substeps` samples per interval (cfs_clearance, include/cfs_hip.h); host arrays in and out.  Returns a
        namespace of (B, nobs) arrays dist_wp (min at the waypoints), dist_path (min over all samples), dist_lower (certified
        lower bound over continuous time), t_path (s) / link_path (1-based) of the first path minimum, and short_by (B,) =
        max_j(margin_j - dist_path[:, j]): how far the motion falls short of the handle's margins (<= 0: it keeps them)."""
        return self._audit(False, False, x_, u, xR1, obs, substeps)

    def alloc_clearance(self, B, device):
        """Device-resident output buffers (torch CUDA tensors) for clearance_device."""
        z = _args.zeros_on(device)
        return SimpleNamespace(**{k: z((B, self.nobs), dt) for k, dt in AUDIT_OUT.items() if k != "tri_path"})

    def clearance_device(self, x_, u, xR1, obs, substeps=16, out=None, stream=None):
        """clearance() on torch CUDA tensors; enqueues on `stream` (default: torch's current stream) and returns without
        synchronising (cfs_clearance_device).  out: an alloc_clearance namespace to write into."""
        return self._audit(False, True, x_, u, xR1, obs, substeps, out, stream)

    def clearance_mesh(self, x_, u, xR1, obs, substeps=16):
        """clearance() for a handle with mesh obstacles (cfs_clearance_mesh, include/cfs_hip.h); host arrays in and out.  The
        (B, nobs) arrays are in the handle's obstacle order (lines first, then the meshes): dist_wp, dist_path, dist_lower,
        t_path, link_path as in clearance(), and tri_path, the index in the caller's triangle list of a closest triangle at the
        dist_path sample (-1 in line columns); short_by (B,) = max_j(margin_j - dist_path[:, j]) over all columns."""
        return self._audit(True, False, x_, u, xR1, obs, substeps)

    def alloc_clearance_mesh(self, B, device):
        """Device-resident output buffers (torch CUDA tensors) for clearance_mesh_device."""
        out = self.alloc_clearance(B, device)
        out.tri_path = torch.zeros(B, self.nobs, dtype=torch.int32, device=device)
        return out

    def clearance_mesh_device(self, x_, u, xR1, obs, substeps=16, out=None, stream=None):
        """clearance_mesh() on torch CUDA tensors; enqueues on `stream` (default: torch's current stream) and returns without
        synchronising (cfs_clearance_mesh_device).  out: an alloc_clearance_mesh namespace to write into."""
        return self._audit(True, True, x_, u, xR1, obs, substeps, out, stream)

    def clearance_mesh_motion(self, x_, u, xR1, obs, substeps=16):
        """clearance_mesh() for a handle whose meshes move (set_mesh_motion; cfs_clearance_mesh_motion, include/cfs_hip.h): the
        same namespace.  Between two waypoints each mesh turns about one axis at a constant rate while the centre of its
        bounding box travels a straight line, and dist_lower carries the mesh's surface speed; a handle with static meshes gives
        clearance_mesh's results bit for bit."""
        return self._audit(True, False, x_, u, xR1, obs, substeps, motion=True)

    def clearance_mesh_motion_device(self, x_, u, xR1, obs, substeps=16, out=None, stream=None):
        """clearance_mesh_motion() on torch CUDA tensors; enqueues on `stream` (default: torch's current stream) and returns
        without synchronising (cfs_clearance_mesh_motion_device).  out: an alloc_clearance_mesh namespace to write into."""
        return self._audit(True, True, x_, u, xR1, obs, substeps, out, stream, motion=True)

    def _margin_on(self, device):
        """the handle's margins as a tensor on `device` (uploaded once: no copy is enqueued by later audits)"""
        cache = self.__dict__.setdefault("_margin_dev", {})
        if device not in cache:
            cache[device] = torch.tensor(self.margin, dtype=torch.float64, device=device)
        return cache[device]

    # ---- CHOMP (row f4) ------------------------------------------------------------------------------------
    def chomp(self, x_init, xR1, ff, caug, obs, u0, D, epsilon):
        """CHOMP_FANUC.optimizer() for B problems (cfs_chomp_batch); host arrays in and out."""
        if self.obstacle_motion == "per_waypoint":
            raise ValueError("CHOMP_FANUC takes static obstacles only: this handle is per-waypoint")
        x_init, xR1, ff, caug, obs, u0 = _f64(x_init), _f64(xR1), _f64(ff), _f64(caug).reshape(-1), _f64(obs), _f64(u0)
        D, epsilon = _f64(np.asarray(D, float).reshape(-1)), _f64(np.asarray(epsilon, float).reshape(-1))
        B = x_init.shape[0]
        assert x_init.shape == (B, self.nx) and u0.shape == (B, self.nn) and obs.shape == (B, self.nobs, 6)
        assert D.size == self.nobs and epsilon.size == self.nobs
        r = self._outputs(B)
        i, o = _batch_in(B, x_init, xR1, ff, caug, obs), _args.fill(_lib.cfs_batch_out(), r)
        _lib.check(self._lib.cfs_chomp_batch(self._h, C.byref(i), _ptr(u0), _ptr(D), _ptr(epsilon), C.byref(o)))
        return r

    # ---- per-problem setup on the device (row f2) ------------------------------------------------------
    def set_state_cost(self, Qaug):
        """The drivers' state-cost matrix Qaug (main_FANUC.m:79-84), once per handle."""
        q = np.asfortranarray(Qaug, dtype=np.float64)
        assert q.shape == (self.nx, self.nx)
        _lib.check(self._lib.cfs_set_state_cost(self._h, _ptr(q)))

    def _terms(self, B, device, stream):
        """((x_init, xR1, ff, caug) uninitialised on `device`, the tail of a build_terms*_device call: their pointers and the stream)"""
        z = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=device)  # noqa: E731
        terms = z(B, self.nx), z(B, self.ns), z(B, self.nn), z(B)
        return terms, [_ptr(t) for t in terms] + [C.c_void_p(_args.stream_ptr(stream, device))]

    def build_terms_device(self, x0, xg, stream=None):
        """(x_init, xR1, ff, caug) as CUDA tensors for B (start, goal) pairs given as CUDA tensors (B, njoint)."""
        B = x0.shape[0]
        assert x0.is_cuda and xg.is_cuda and x0.dtype == torch.float64 and x0.is_contiguous() and xg.is_contiguous()
        terms, tail = self._terms(B, x0.device, stream)
        _lib.check(self._lib.cfs_build_terms_device(self._h, B, _ptr(x0), _ptr(xg), *tail))
        return terms

    def build_terms_from_routes_device(self, routes, stream=None):
        """(x_init, xR1, ff, caug) for B RRT routes given as a CUDA tensor (B, nwp, njoint): cubic zero-velocity
        resampling to H+1 samples + cost terms, on the device (RRTstar_CFS.m:94-110, 159-163)."""
        B, nwp = routes.shape[0], routes.shape[1]
        assert routes.is_cuda and routes.dtype == torch.float64 and routes.is_contiguous() and routes.shape[2] == self.nj
        terms, tail = self._terms(B, routes.device, stream)
        _lib.check(self._lib.cfs_build_terms_from_routes_device(self._h, B, _ptr(routes), nwp, *tail))
        return terms

    def build_terms_from_ragged_routes_device(self, routes, nwp, stream=None):
        """The same for routes of different lengths as cfs_rrt_grow_device leaves them: routes (B, nwp_stride, njoint) CUDA
        float64, nwp (B,) CUDA int32 rows used per route (cfs_build_terms_from_ragged_routes_device)."""
        B, stride = routes.shape[0], routes.shape[1]
        assert routes.is_cuda and routes.dtype == torch.float64 and routes.is_contiguous() and routes.shape[2] == self.nj
        assert nwp.is_cuda and nwp.dtype == torch.int32 and nwp.is_contiguous() and nwp.shape == (B,)
        terms, tail = self._terms(B, routes.device, stream)
        _lib.check(self._lib.cfs_build_terms_from_ragged_routes_device(self._h, B, _ptr(routes), stride, _ptr(nwp), *tail))
        return terms

    # ---- measurement ------------------------------------------------------------------------------
    def profile(self, on=True):
        _lib.check(self._lib.cfs_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """(ms in the fused solve kernel, ms in the MFMA batched product, solves) since the last read;
        HIP events on the stream the kernels were launched on."""
        a, b, n = C.c_double(0), C.c_double(0), C.c_int(0)
        _lib.check(self._lib.cfs_profile_read(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    # ---- EVAL (Lib/EVAL.m:51-53, 75-78) ------------------------------------------------------------------
    def cost_b(self, ff, caug, want_u=False):
        """Cost_b = get_Cost_b() for B problems: cost of the unconstrained minimiser -H^{-1} ff (cfs_cost_b)."""
        ff, caug = _f64(np.atleast_2d(ff)), _f64(caug).reshape(-1)
        B = ff.shape[0]
        assert ff.shape == (B, self.nn) and caug.shape == (B,)
        cost = np.zeros(B)
        ub = np.zeros((B, self.nn)) if want_u else None
        _lib.check(self._lib.cfs_cost_b(self._h, B, _ptr(ff), _ptr(caug), _ptr(cost), _ptr(ub)))
        return (cost, ub) if want_u else cost

    def get_cost(self, u, ff, caug):
        """get_cost(u) = 0.5 u'QQ u + ff'u + caug for B given u (cfs_get_cost)."""
        u, ff, caug = _f64(np.atleast_2d(u)), _f64(np.atleast_2d(ff)), _f64(caug).reshape(-1)
        B = u.shape[0]
        assert u.shape == (B, self.nn) and ff.shape == (B, self.nn) and caug.shape == (B,)
        cost = np.zeros(B)
        _lib.check(self._lib.cfs_get_cost(self._h, B, _ptr(u), _ptr(ff), _ptr(caug), _ptr(cost)))
        return cost

    # ---- developer / test switches (cfs_debug_*, per handle) ---------------------------------------------
    def debug_options(self, warm_max=0, polish_tol=0.0, **flags):
        """cfs_debug_set_options: flags from _lib.DBG (no_refine, no_warm_start, no_certificate, no_prune, no_auto_order,
        tier_w1, clear_no_bound, clear_seed); no flags = the defaults."""
        mask = 0
        for k, v in flags.items():
            if v:
                mask |= _lib.DBG[k]
        _lib.check(self._lib.cfs_debug_set_options(self._h, mask, int(warm_max), float(polish_tol)))

    def stamps(self, B=None):
        """B given: enable the cycle stamps for the next solves of <= B problems (0: off); B None: read them, (n, 12) uint64."""
        if B is not None:
            _lib.check(self._lib.cfs_debug_stamps(self._h, int(B), None))
            self._stamps_B = int(B)
            return None
        out = np.zeros((self._stamps_B, 12), np.uint64)
        _lib.check(self._lib.cfs_debug_stamps(self._h, self._stamps_B, _ptr(out)))
        return out

    def trace(self, b=None, cap=0):
        """b given: trace the active-set steps of problem b (cap records; cap 0: off); b None: read, (n, 8) float64."""
        if b is not None:
            _lib.check(self._lib.cfs_debug_trace_begin(self._h, int(b), int(cap)))
            self._trace_cap = int(cap)
            return None
        buf = np.zeros((self._trace_cap + 1) * 8)
        _lib.check(self._lib.cfs_debug_trace_read(self._h, _ptr(buf)))
        return buf[8:8 + 8 * int(buf[0])].reshape(-1, 8)

    def launch_order_debug(self, x_init, obs):
        """(key, order) of the launch-order pre-pass for these B problems, as a solve would compute them (cfs_debug_launch_order):
        key[b] counts the (waypoint, line obstacle) pairs of x_init[b] closer than the margin, order lists the problems by
        descending key, ties by index."""
        x_init, obs = _f64(x_init), _f64(obs)
        B = x_init.shape[0]
        assert x_init.shape == (B, self.nx)
        self._check_obs(obs, B)
        key, order = np.zeros(B, np.int32), np.zeros(B, np.int32)
        _lib.check(self._lib.cfs_debug_launch_order(self._h, B, _ptr(x_init), _ptr(obs), _ptr(key), _ptr(order)))
        return key, order

    def log_u(self, on=True):
        """log u after every outer iteration of the next solves (either solver; cfs_debug_log_u)."""
        _lib.check(self._lib.cfs_debug_log_u(self._h, 1 if on else 0))

    def read_u_log(self, B):
        out = np.zeros((B, self.K, self.nn))
        _lib.check(self._lib.cfs_debug_read_u_log(self._h, int(B), _ptr(out)))
        return out

    # ---- pieces -----------------------------------------------------------------------------------
    def linearize(self, x_, obs):
        x_, obs = _f64(x_), _f64(obs)
        B = x_.shape[0]
        self._check_obs(obs, B)
        dist = np.zeros((B, self.nobs, self.H))
        lid = np.zeros((B, self.nobs, self.H), np.int32)
        grad = np.zeros((B, self.nobs, self.H, self.nj))
        _lib.check(self._lib.cfs_linearize(self._h, B, _ptr(x_), _ptr(obs), _ptr(dist), _ptr(lid), _ptr(grad)))
        return dist, lid, grad

    def get_con(self, x_, u, xR1, obs):
        x_, u, xR1, obs = _f64(x_), _f64(u), _f64(xR1), _f64(obs)
        B = x_.shape[0]
        self._check_obs(obs, B)
        A = np.zeros((B, self.nn, self.rows))  # per problem rows x nn column-major == (nn, rows) C-order
        b = np.zeros((B, self.rows))
        _lib.check(self._lib.cfs_get_con(self._h, B, _ptr(x_), _ptr(u), _ptr(xR1), _ptr(obs), _ptr(A), _ptr(b)))
        return A.transpose(0, 2, 1), b

    def qp(self, lin, u_lin, xR1, dist, grad, want_lambda=True):
        lin, u_lin, xR1, dist, grad = _f64(lin), _f64(u_lin), _f64(xR1), _f64(dist), _f64(grad)
        B = lin.shape[0]
        u = np.zeros((B, self.nn))
        nlam = self.nobs * self.H + (4 if self.joint_limits() is None else 6) * self.nn
        lam = np.zeros((B, nlam)) if want_lambda else None
        it, st = np.zeros(B, np.int32), np.zeros(B, np.int32)
        _lib.check(self._lib.cfs_qp(self._h, B, _ptr(lin), _ptr(u_lin), _ptr(xR1), _ptr(dist), _ptr(grad), _ptr(u),
                                    _ptr(lam), _ptr(it), _ptr(st)))
        return u, lam, it, st


FUSED_TIERS = ("w1", "w2m", "w2s")


def fused_tier(nj, H, nobs, mode="CFS", per_waypoint=False, limits=False, force_w1=False):
    """cfs_debug_fused_tier: index into FUSED_TIERS of the fused solver's tier that a solve of this shape runs (host only, no
    device); CfsError for a shape no handle can have."""
    tier = C.c_int(-1)
    _lib.check(_lib.lib().cfs_debug_fused_tier(int(nj), int(H), int(nobs), _lib.MODE[mode], int(bool(per_waypoint)), int(bool(limits)),
                                               int(bool(force_w1)), C.byref(tier)))
    return tier.value


def dist_arm(robot, theta, obs_l, want_pos=False, want_grad=False):
    """[d, linkid] = dist_arm_*(theta, base, obs_l, robot) for N configurations x nobs obstacle axes
    (theta: (N, nj); obs_l: (nobs, 6)).  want_grad: also grad (N, nobs, nj), the analytic derivative of d with respect to
    theta (cfs_dist_arm_grad; d and linkid are the same numbers).  Returns (d, linkid[, pos][, grad])."""
    theta, obs_l = _f64(np.atleast_2d(theta)), _f64(np.atleast_2d(obs_l))
    N, nj = theta.shape
    nobs = obs_l.shape[0]
    d = np.zeros((N, nobs))
    lid = np.zeros((N, nobs), np.int32)
    pos = np.zeros((N, nj, 2, 3)) if want_pos else None
    rb = to_c_robot(robot)
    grad = np.zeros((N, nobs, nj)) if want_grad else None
    if want_grad:
        _lib.check(_lib.lib().cfs_dist_arm_grad(C.byref(rb), nj, N, _ptr(theta), nobs, _ptr(obs_l), _ptr(d), _ptr(lid), _ptr(grad)))
    if want_pos or not want_grad:
        _lib.check(_lib.lib().cfs_dist_arm(C.byref(rb), nj, N, _ptr(theta), nobs, _ptr(obs_l), _ptr(d), _ptr(lid), _ptr(pos)))
    return (d, lid) + ((pos,) if want_pos else ()) + ((grad,) if want_grad else ())


class EVAL:
    """Lib/EVAL.m: ``eval = EVAL(sys_info)``, ``Cost_b = eval.get_Cost_b()`` (main_FANUC.m:131-132), ``get_cost(u)``,
    ``store_result(u)``, ``stop_outer(iter_O)`` with the reference's field names (:9-37).  The two cost functions run in
    libcfs_hip.so (cfs_cost_b, cfs_get_cost: QQ*u on the matrix cores); the stop test and the history appends are the
    reference's host-side bookkeeping.  Inside ``optimizer()`` all of this happens in the fused kernel; the methods are for
    callers that use EVAL on its own, as main_FANUC.m does for the baseline cost."""

    def __init__(self, sys_info, device=None):
        self.sys_info = sys_info
        self.epsilon_O, self.MAX_O_ITER = sys_info.epsilon_O, sys_info.MAX_O_ITER     # EVAL.m:43-44
        self.x_ = np.asarray(sys_info.x_, float).reshape(-1).copy()                   # :46
        self.x_old = np.ones_like(self.x_)                                            # :47
        self.u_old = None
        self.Cost_b = 0.0
        self.total_iter = 0
        self.cost_old, self.cost_new = 100000.0, 0.0                                  # :29-30
        self.cost_all, self.e_cost_all, self.e_u_all = np.zeros(0), np.zeros(0), np.zeros(0)
        self._device, self._batch = device, None

    def _family(self):
        if self._batch is None:      # the family handle (QQ and its inverse on the device); obstacles play no role in the costs
            self._batch = CFSBatch(self.sys_info, 1, [0.0], mode="CFS", max_batch=1, device=self._device)
        return self._batch

    def get_cost(self, u):
        """cost = 0.5*u'*Qaug*u + paug'*u + caug with the drivers' Qaug = QQ, paug = ff (EVAL.m:51-53, main_FANUC.m:110-112)."""
        s = self.sys_info
        return float(self._family().get_cost(np.asarray(u, float).reshape(1, -1), _f64(s.ff).reshape(1, -1), np.array([s.caug], float))[0])

    def get_Cost_b(self):
        """cost of the unconstrained QP's minimiser (EVAL.m:75-78)."""
        s = self.sys_info
        self.Cost_b = float(self._family().cost_b(_f64(s.ff).reshape(1, -1), np.array([s.caug], float))[0])
        return self.Cost_b

    def store_result(self, u):
        """EVAL.m:55-59."""
        u = np.asarray(u, float).reshape(-1)
        u_old = np.zeros_like(u) if self.u_old is None else np.asarray(self.u_old, float).reshape(-1)
        self.cost_all = np.append(self.cost_all, self.cost_new)
        self.e_cost_all = np.append(self.e_cost_all, abs(self.cost_old - self.cost_new))
        self.e_u_all = np.append(self.e_u_all, float(np.linalg.norm(u_old - u)))
        return self

    def stop_outer(self, iter_O):
        """EVAL.m:61-73: stop when ||x_ - x_old|| < epsilon_O or iter_O > MAX_O_ITER."""
        stop = False
        if float(np.linalg.norm(np.asarray(self.x_, float).reshape(-1) - np.asarray(self.x_old, float).reshape(-1))) < self.epsilon_O:
            print(f"Converged at step{iter_O}")
            stop = True
        if iter_O > self.MAX_O_ITER:
            print("MAX_ITER")
            stop = True
        return stop


class _SolverBase:
    MODE = "CFS"
    MARGIN_KEY = "epsilon"

    def __init__(self, obs, sys_info, ROBOT="M16iB", device=None, jacobian="fd_literal", on_infeasible="stop", soft_weight=None,
                 joint_limits=None, audit=None, audit_mesh=None, audit_mesh_motion=None):
        """jacobian: "fd_literal" (num_jac.m, the default) | "analytic" (CFSBatch).
        audit: None (the default: results are exactly those without the argument) | an integer S in 1..64: after optimizer(),
        .clearance holds CFSBatch.clearance of the returned trajectory with S sub-steps per interval (its one problem: arrays of
        shape (nobs,), short_by a float); line obstacles only.
        audit_mesh: the same for an obs cell with at least one mesh: None (the default) | S in 1..64: after optimizer(),
        .clearance_mesh holds CFSBatch.clearance_mesh of the returned trajectory (all columns, lines first, with tri_path).
        audit_mesh_motion: None (the default) | S in 1..64: after optimizer(), .clearance_mesh_motion holds
        CFSBatch.clearance_mesh_motion of the returned trajectory; the one audit that takes mesh entries with a "pose".
        joint_limits: None (the default) | "robot" | an (njoint, 2) array of [lo, hi] (CFSBatch); get_con then has the position rows.
        on_infeasible: "stop" (the default) | "soften" with soft_weight= (CFSBatch); after optimizer(), viol_all and n_soft.
        obs{j}["l"] may be 3x2xH (shape (3, 2, H): the obstacle's axis at waypoints 1..H); any such entry makes the handle
        per-waypoint, and the 3x2 entries are then held over the horizon (obs_traj_to_array).
        A mesh entry may carry "pose" (mesh_pose_array: the rigid pose of the mesh at waypoints 1..H); mesh entries without one
        are then held still, the line obstacles of such a cell are static, and audit_mesh= is refused."""
        _args.code(_lib.JACOBIAN, jacobian, "jacobian")
        _infeasible_args(on_infeasible, soft_weight)
        _joint_limits_array(joint_limits, sys_info.robot, int(sys_info.njoint))
        self.audit = None if audit is None else _args.int_in(audit, "audit", 1, 64)
        meshes = obs_meshes(obs, poses=True)
        if self.audit is not None and meshes:
            raise ValueError("audit= measures line obstacles only: the obs cell holds mesh obstacles")
        self.clearance = None
        self.audit_mesh = None if audit_mesh is None else _args.int_in(audit_mesh, "audit_mesh", 1, 64)
        if self.audit_mesh is not None and not meshes:
            raise ValueError("audit_mesh= needs an obs cell with at least one mesh obstacle: audit= measures line obstacles")
        self.clearance_mesh = None
        self.audit_mesh_motion = None if audit_mesh_motion is None else _args.int_in(audit_mesh_motion, "audit_mesh_motion", 1, 64)
        if self.audit_mesh_motion is not None and not meshes:
            raise ValueError("audit_mesh_motion= needs an obs cell with at least one mesh obstacle: audit= measures line obstacles")
        self.clearance_mesh_motion = None
        self._mesh_poses = obs_mesh_poses(obs, sys_info.H)   # checked before anything touches the device
        if self.audit_mesh is not None and self._mesh_poses is not None:
            raise ValueError("audit_mesh= audits static meshes: a mesh entry of the obs cell carries a pose")
        if on_infeasible == "soften" and meshes:
            raise ValueError('on_infeasible="soften" does not support mesh obstacles')
        self._moving = obs_moving(obs)
        if self._moving:
            if meshes:
                raise ValueError("mesh obstacles are static: an obs cell with 3x2xH axes cannot hold meshes")
            obs_traj_to_array(obs, sys_info.H)          # shapes checked before anything touches the device
        self.obs, self.sys_info, self.ROBOT = obs, sys_info, ROBOT
        if getattr(sys_info.robot, "name", ROBOT) != ROBOT:
            raise ValueError(f"sys_info.robot is {sys_info.robot.name!r} but ROBOT={ROBOT!r}")
        self.nn = sys_info.H * sys_info.nu
        self.x_ = np.asarray(sys_info.x_, float).reshape(-1).copy()
        self.u = np.zeros(self.nn)
        self.Ainq = self.binq = None
        self.eval = EVAL(sys_info)
        self.iter_O, self.total_iter, self.status = 1, 0, None
        self._batch = CFSBatch(sys_info, len(obs), [o[self.MARGIN_KEY] for o in obs], mode=self.MODE, max_batch=1,
                               device=device, jacobian=jacobian, on_infeasible=on_infeasible, soft_weight=soft_weight,
                               obstacles="per_waypoint" if self._moving else "static", joint_limits=joint_limits)
        self.viol_all, self.n_soft = np.zeros(0), 0
        if meshes:
            self._batch.set_meshes(meshes)
        if self._mesh_poses is not None:
            self._batch.set_mesh_motion(self._mesh_poses)

    def _args(self):
        s = self.sys_info
        xR1 = np.asarray(s.xR, float).reshape(s.nstate, -1)[:, 0]
        obs = obs_traj_to_array(self.obs, s.H) if self._moving else obs_to_array(self.obs)
        return xR1[None], _f64(s.ff).reshape(1, -1), np.array([s.caug], float), obs[None]

    def get_con(self):
        """self.Ainq / self.binq at the current (x_, u): dense, reference row order."""
        xR1, _, _, obs = self._args()
        A, b = self._batch.get_con(self.x_[None], self.u[None], xR1, obs)
        self.Ainq, self.binq = A[0], b[0]
        return self

    def optimizer(self, noise=None):
        xR1, ff, caug, obs = self._args()
        nz = None if noise is None else _f64(noise)[None]
        r = self._batch.solve(np.asarray(self.sys_info.x_, float).reshape(1, -1), xR1, ff, caug, obs, noise=nz)
        n = int(r.iter_O[0]) - 1
        self.u, self.x_ = r.u[0], r.x_[0]
        self.iter_O, self.total_iter, self.status = int(r.iter_O[0]), int(r.total_iter[0]), int(r.status[0])
        self.eval.cost_all, self.eval.e_cost_all, self.eval.e_u_all = r.cost_all[0, :n], r.e_cost_all[0, :n], r.e_u_all[0, :n]
        self.viol_all, self.n_soft = r.viol_all[0, :n], int(r.n_soft[0])
        self.eval.cost_new = float(r.cost_all[0, n - 1]) if n > 0 else float(self.sys_info.caug)
        self.eval.x_ = self.x_
        row0 = lambda c: SimpleNamespace(**{k: float(v[0]) if v.ndim == 1 else v[0] for k, v in vars(c).items()})  # noqa: E731
        if self.audit is not None:                       # the one problem's row of every field; short_by (B,) becomes a float
            self.clearance = row0(self._batch.clearance(r.x_, r.u, xR1, obs, substeps=self.audit))
        if self.audit_mesh is not None:
            self.clearance_mesh = row0(self._batch.clearance_mesh(r.x_, r.u, xR1, obs, substeps=self.audit_mesh))
        if self.audit_mesh_motion is not None:
            self.clearance_mesh_motion = row0(self._batch.clearance_mesh_motion(r.x_, r.u, xR1, obs, substeps=self.audit_mesh_motion))
        if self.status == 0:
            print(f"Converged at step{self.iter_O}")  # EVAL.m:66
        elif self.status == 1:
            print("MAX_ITER")  # EVAL.m:70
        return self


class CFS_FANUC(_SolverBase):
    """Lib/CFS_FANUC.m -- margin obs{j}.epsilon, QP with QQ/ff and +-MAX_input bounds."""
    MODE, MARGIN_KEY = "CFS", "epsilon"


class PSGCFS_FANUC(_SolverBase):
    """Lib/PSGCFS_FANUC.m -- margin obs{j}.D, noisy gradient step + projection.  The normrnd draws
    (PSGCFS_FANUC.m:109) are passed in explicitly: optimizer(noise=(rows, nn) array of N(0, 0.1^2))."""
    MODE, MARGIN_KEY = "PSGCFS", "D"


class CHOMP_FANUC:
    """Lib/CHOMP_FANUC.m -- ``CHOMP_FANUC(obs_, sys_info, uref, ROBOT).optimizer()``.  ``obs_`` is the reference's cell:
    ``obs_[0] = dict(num_obs=n)`` followed by the n obstacles (``l``, ``D``, ``epsilon``) (M16iB/CHOMP.m:26-29)."""

    def __init__(self, obs, sys_info, uu, ROBOT="M16iB", device=None, audit=None, audit_mesh=None, audit_mesh_motion=None):
        if audit_mesh_motion is not None:
            raise ValueError("CHOMP_FANUC has no clearance audit: audit_mesh_motion= is an option of CFS_FANUC and PSGCFS_FANUC")
        if audit is not None:
            raise ValueError("CHOMP_FANUC has no clearance audit: audit= is an option of CFS_FANUC and PSGCFS_FANUC")
        if audit_mesh is not None:
            raise ValueError("CHOMP_FANUC has no clearance audit: audit_mesh= is an option of CFS_FANUC and PSGCFS_FANUC")
        self.obs, self.sys_info, self.ROBOT = obs, sys_info, ROBOT
        if getattr(sys_info.robot, "name", ROBOT) != ROBOT:
            raise ValueError(f"sys_info.robot is {sys_info.robot.name!r} but ROBOT={ROBOT!r}")
        n = int(obs[0]["num_obs"])
        self._obstacles = list(obs[1:1 + n])
        if obs_moving(self._obstacles):
            raise ValueError("CHOMP_FANUC takes static obstacles only: obs_{j}.l must be 3x2")
        self.nn = sys_info.H * sys_info.nu
        self.x_ = np.asarray(sys_info.x_, float).reshape(-1).copy()
        self.u = np.asarray(uu, float).reshape(-1).copy()
        self.eval = EVAL(sys_info)
        self.iter_O, self.total_iter = 1, 0
        self._batch = CFSBatch(sys_info, n, [o["epsilon"] for o in self._obstacles], mode="CFS", max_batch=1, device=device)

    def optimizer(self):
        s = self.sys_info
        xR1 = np.asarray(s.xR, float).reshape(s.nstate, -1)[:, 0]
        r = self._batch.chomp(np.asarray(s.x_, float).reshape(1, -1), xR1[None], _f64(s.ff).reshape(1, -1), np.array([s.caug], float),
                              obs_to_array(self._obstacles)[None], self.u[None], [o["D"] for o in self._obstacles],
                              [o["epsilon"] for o in self._obstacles])
        n = int(r.iter_O[0]) - 1
        self.u, self.x_, self.iter_O = r.u[0], r.x_[0], int(r.iter_O[0])
        self.eval.cost_all, self.eval.e_cost_all, self.eval.e_u_all = r.cost_all[0, :n], r.e_cost_all[0, :n], r.e_u_all[0, :n]
        if n > 0:
            self.eval.cost_new = float(r.cost_all[0, n - 1])
        print("MAX_ITER")  # EVAL.m:70 (the loop never converges by distance: eval.x_ is not refreshed)
        return self
