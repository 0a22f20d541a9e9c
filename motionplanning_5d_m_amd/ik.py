"""Cartesian goals: batched collision-aware inverse kinematics over ``cfs_ik_solve`` (include/cfs_hip.h, "inverse kinematics").

The reference's drivers type their goals in as joint vectors (``xg``, main_FANUC.m:30, RRTstar_CFS.m:43).  ``IKSolver`` turns T
Cartesian targets -- a point for the tool, optionally a direction for its axis -- into goal configurations inside the joint
ranges (``robot.thetamax``) that RRT's ``feasible()`` (Lib/RRT_FANUC.m:146-181) accepts against the line obstacles, each the
nearest such configuration to a reference pose.  One wavefront per target, one lane per restart; this module packs arguments
and unpacks results, the iteration and the selection are HIP kernels (csrc/cfs_ik.hip).

The tool defaults to the reference's end effector: ``tool = robot.cap{njoint}.p(:,1)`` (``all_ee``, Lib/RRT_FANUC.m:186) and
``tool_axis = unit(p(:,2) - p(:,1))`` of the same capsule.

Mesh obstacles: the obs cell may end with ``dict(mesh=Mesh, D=...)`` entries (after the line obstacles, the convention of
``RRT_FANUC`` and ``solvers.obs_meshes``).  A converged restart that passed the lines is then also rejected when a link axis comes
closer to mesh j than ``max(D_j, 1e-4)`` -- the decision of ``cfs_rrt_grow_mesh`` -- and ``solve`` / ``solve_device`` route to
``cfs_ik_solve_mesh*`` (include/cfs_hip.h).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _args, _lib
from ._args import f64 as _f64, is_int as _is_int, ptr as _ptr
from .robotproperty2 import to_c_robot
from .mesh import Mesh
from .solvers import _joint_limits_array

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_RESTARTS = 64            # one wavefront lane per restart
MAX_ITER = 1000


def _vec3(v, name, nonzero=False):
    try:
        a = np.array(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be 3 numbers, not {v!r}") from None
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be 3 finite numbers, not {v!r}")
    if nonzero and not np.linalg.norm(a) > 0:
        raise ValueError(f"{name} must not be zero")
    return a


def _njoint(robot, njoint):
    ncap = len(robot.cap)
    if njoint is None:                                        # the joints the reference's drivers plan: 5 of the M200i's 6 (nstate = 5)
        njoint = 5 if robot.name == "M200i" else min(int(robot.nlink), ncap, 6)
    if not _is_int(njoint) or not 2 <= njoint <= min(6, int(robot.nlink), ncap):
        raise ValueError(f"njoint must be an integer in 2..{min(6, int(robot.nlink), ncap)} for robot {robot.name!r}, not {njoint!r}")
    return int(njoint)


def default_tool(robot, njoint):
    """(tool, tool_axis) of the reference's end effector: cap{njoint}.p(:,1) and the unit vector towards p(:,2); a capsule of zero
    length (both end points equal) gives the link frame's z axis."""
    cp = robot.cap[njoint - 1]
    p = np.asarray(cp.p if hasattr(cp, "p") else cp["p"], dtype=np.float64)
    d = p[:, 1] - p[:, 0]
    n = np.linalg.norm(d)
    return p[:, 0].copy(), (d / n if n > 0 else np.array([0.0, 0.0, 1.0]))


def tool_pose(robot, theta, njoint=None, tool=None, tool_axis=None, want_jac=False):
    """cfs_tool_pose: world position of `tool` and world direction of `tool_axis` (both in the frame of link njoint; defaults:
    default_tool) for N configurations theta (N, njoint).  Returns (pos (N, 3), dir (N, 3)[, jac (N, 6, njoint)]); jac is the
    analytic Jacobian the solver uses, rows 0-2 of the position, rows 3-5 of the direction."""
    theta = _f64(np.atleast_2d(theta))
    njoint = _njoint(robot, theta.shape[1] if njoint is None else njoint)
    if theta.ndim != 2 or theta.shape[1] != njoint:
        raise ValueError(f"theta must have shape (N, {njoint}), not {theta.shape}")
    t0, a0 = default_tool(robot, njoint)
    tool = t0 if tool is None else _vec3(tool, "tool")
    tool_axis = a0 if tool_axis is None else _vec3(tool_axis, "tool_axis", nonzero=True)
    N = theta.shape[0]
    pos, dr = np.zeros((N, 3)), np.zeros((N, 3))
    jac = np.zeros((N, 6, njoint)) if want_jac else None
    rb = to_c_robot(robot)
    _lib.check(_lib.lib().cfs_tool_pose(C.byref(rb), njoint, _ptr(_f64(tool)), _ptr(_f64(tool_axis)), N, _ptr(theta), _ptr(pos), _ptr(dr),
                                        _ptr(jac)))
    return (pos, dr, jac) if want_jac else (pos, dr)


class _ToolSolver:
    """What IKSolver and CartesianPath share: the chain (robot, njoint, joint ranges, tool point and axis), the tolerances and the
    weight, the obstacles, the device, the checks of the targets and the plumbing of their device entries."""

    def __init__(self, robot, obs, joint_limits, tool, tool_axis, tol_pos, tol_axis, weight, device, njoint):
        self.robot, self.nj = robot, _njoint(robot, njoint)
        nj = self.nj
        if joint_limits is None:
            raise ValueError('joint_limits must be "robot" or an (njoint, 2) array: inverse kinematics needs finite joint ranges')
        lim = _joint_limits_array(joint_limits, robot, nj)
        if not np.isfinite(lim).all():
            raise ValueError("joint_limits must be finite")
        self.lo, self.hi = _f64(lim[:, 0]), _f64(lim[:, 1])
        t0, a0 = default_tool(robot, nj)
        self.tool = t0 if tool is None else _vec3(tool, "tool")
        self.tool_axis = a0 if tool_axis is None else _vec3(tool_axis, "tool_axis", nonzero=True)
        self.tool_axis = self.tool_axis / np.linalg.norm(self.tool_axis)
        self.tol_pos, self.tol_axis = _args.real(tol_pos, "tol_pos"), _args.real(tol_axis, "tol_axis")
        if weight is None:
            self.weight = None
        else:
            try:
                w = np.array(weight, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError(f"weight must be {nj} numbers, not {weight!r}") from None
            if w.shape != (nj,) or not np.isfinite(w).all() or not (w > 0).all():
                raise ValueError(f"weight must be {nj} finite numbers > 0, not {weight!r}")
            self.weight = _f64(w)
        obs = [] if obs is None else list(obs)
        if len(obs) > _lib.CFS_MAX_OBS:
            raise ValueError(f"{len(obs)} obstacles: at most {_lib.CFS_MAX_OBS}")
        _args.obs_meshes(obs)                                 # ValueError when a mesh precedes a line obstacle
        for j, o in enumerate(obs):                           # the meshes first, then the lines
            if "mesh" not in o:
                continue
            if not isinstance(o["mesh"], Mesh):
                raise ValueError(f"obs[{j}]['mesh'] must be a Mesh, not {type(o['mesh']).__name__}")
            _args.real(o.get("D"), f"obs[{j}]['D'] (a mesh obstacle)")
        for j, o in enumerate(obs):
            if "mesh" in o:
                continue
            if np.shape(o["l"]) != (3, 2) or not np.isfinite(np.asarray(o["l"], float)).all():
                raise ValueError(f"obs[{j}]['l'] must be a finite 3x2 array")
            _args.real(o.get("D"), f"obs[{j}]['D']", positive=False)
        self.obs, self.D, self._meshes, self._D_mesh = _args.split_obs(obs)
        if device is not None:
            if torch is None:
                raise ValueError("device= needs torch")
            device = _args.cuda_device(device)
        self.device = device
        self._dev = None                                      # (device, obstacle rows, D) uploaded by the device entry

    def _targets(self, target_pos, target_axis, theta_ref):
        """host arrays (T, 3), (T, 3) | None, (T, nj), validated"""
        nj = self.nj
        try:
            tp = np.array(target_pos, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("target_pos must be an array of shape (T, 3) or (3,)") from None
        if tp.ndim == 1:
            tp = tp[None, :]
        if tp.ndim != 2 or tp.shape[1] != 3 or tp.shape[0] < 1:
            raise ValueError(f"target_pos must have shape (T, 3) with T >= 1 or (3,), not {tp.shape}")
        if not np.isfinite(tp).all():
            raise ValueError("target_pos must be finite")
        T = tp.shape[0]
        ta = None
        if target_axis is not None:
            ta = np.array(target_axis, dtype=np.float64)
            if ta.ndim == 1:
                ta = np.broadcast_to(ta[None, :], (T, ta.shape[0]))
            if ta.shape != (T, 3):
                raise ValueError(f"target_axis must have shape ({T}, 3) or (3,), not {ta.shape}")
            if not np.isfinite(ta).all():
                raise ValueError("target_axis must be finite")
            if not (np.linalg.norm(ta, axis=1) > 0).all():
                raise ValueError("a target_axis row is zero")
        return T, _f64(tp), (None if ta is None else _f64(ta)), self._ref(theta_ref, T)

    def _ref(self, theta_ref, T):
        """the host array (T, nj) of theta_ref, validated; None: the middle of the joint ranges"""
        nj = self.nj
        if theta_ref is None:
            tr = np.broadcast_to(0.5 * (self.lo + self.hi)[None, :], (T, nj))
        else:
            tr = np.array(theta_ref, dtype=np.float64)
            if tr.ndim == 1:
                tr = np.broadcast_to(tr[None, :], (T, tr.shape[0]))
            if tr.shape != (T, nj):
                raise ValueError(f"theta_ref must have shape ({T}, {nj}) or ({nj},), not {tr.shape}")
            if not np.isfinite(tr).all():
                raise ValueError("theta_ref must be finite")
        return _f64(tr)

    def _fill_desc(self, d, use_axis, obs, D):
        """the fields cfs_ik_desc and cfs_cart_desc share"""
        d.robot = to_c_robot(self.robot)
        d.njoint, d.use_axis = self.nj, int(use_axis)
        for q in range(3):
            d.tool[q], d.tool_axis[q] = float(self.tool[q]), float(self.tool_axis[q])
        d.lo, d.hi, d.weight = _ptr(self.lo), _ptr(self.hi), _ptr(self.weight)
        d.tol_pos, d.tol_axis = self.tol_pos, self.tol_axis
        d.nobs = int(self.obs.shape[0])
        d.obs, d.D = (_ptr(obs), _ptr(D)) if d.nobs else (None, None)
        return d

    def _results(self, shapes, want_candidates, dev=None):
        """the result namespace of a shapes table (field -> (shape, dtype), in the order of the out struct; the cand_ fields only
        with want_candidates): numpy arrays, or tensors on `dev`"""
        z = _args.zeros_on(dev)
        return SimpleNamespace(**{k: z(*sd) for k, sd in shapes.items() if want_candidates or not k.startswith("cand_")})

    # ---- the device entries: what follows the check of the first tensor, whose device `dev` is the launch's -------------
    def _theta_ref(self, theta_ref, T, dev):
        if theta_ref is None:
            return torch.tensor(0.5 * (self.lo + self.hi), dtype=torch.float64, device=dev).unsqueeze(0).expand(T, -1).contiguous()
        return _args.cuda_tensor(theta_ref, "theta_ref", (T, self.nj), device=dev)

    def _on(self, dev, stream):
        """(the torch stream of the launch, obstacle rows on dev, their D on dev); the obstacles are uploaded once per device"""
        stream = _args.as_stream(stream, dev)
        if self._dev is None or self._dev[0] != dev:
            self._dev = (dev, torch.tensor(self.obs, dtype=torch.float64, device=dev), torch.tensor(self.D, dtype=torch.float64, device=dev))
        return stream, self._dev[1], self._dev[2]

    def _record(self, stream, *tensors):
        for t in tensors + self._dev[1:]:
            if t is not None:
                t.record_stream(stream)


class IKSolver(_ToolSolver):
    """Batched inverse kinematics for one robot, one set of obstacles and one set of joint ranges.

    robot: robotproperty2(id).  obs: None or an obs cell of line obstacles (dict(l=3x2, D=...)), which may end with mesh obstacles
    (dict(mesh=Mesh, D=...), D finite and > 0); a mesh before a line obstacle is refused.  mesh_variant: None (the library's
    default) or a key of _lib.IK_MESH ("per_lane" | "wave" | "small_frontier"): the developer switch of cfs_ik_solve_mesh*, with
    bit-identical results under every value.
    joint_limits: "robot" (robot.thetamax[:njoint]) or an (njoint, 2) array of finite [lo, hi].  tool / tool_axis: a point and a
    direction in the frame of link njoint (defaults: default_tool).  restarts: 1..64 starts per target, restart 0 at theta_ref,
    the others drawn in the joint ranges from `seed`.  tol_pos (m) / tol_axis (norm of the difference of unit vectors): what
    "reached" means.  weight: njoint weights > 0 of the distance to theta_ref (None: ones).  njoint: joints of the chain (default: 5
    for the M200i, the joints the reference plans; otherwise every link that has a capsule, at most 6).
    Arguments are validated here, before anything touches the device."""

    def __init__(self, robot, obs=None, joint_limits="robot", tool=None, tool_axis=None, restarts=64, max_iter=100, tol_pos=1e-6,
                 tol_axis=1e-6, weight=None, device=None, njoint=None, mesh_variant=None):
        super().__init__(robot, obs, joint_limits, tool, tool_axis, tol_pos, tol_axis, weight, device, njoint)
        self.restarts = _args.int_in(restarts, "restarts", 1, MAX_RESTARTS)
        self.max_iter = _args.int_in(max_iter, "max_iter", 1, MAX_ITER)
        self.mesh_variant = None if mesh_variant is None else _args.one_of(_lib.IK_MESH, mesh_variant, "mesh_variant")

    def _desc(self, use_axis, seed, obs, D):
        d = self._fill_desc(_lib.cfs_ik_desc(), use_axis, obs, D)
        d.restarts, d.max_iter, d.seed = self.restarts, self.max_iter, seed
        return d

    def _shapes(self, T):
        nj, R = self.nj, self.restarts
        f, i = np.float64, np.int32
        return dict(theta=((T, nj), f), status=((T,), i), selected=((T,), i), n_ok=((T,), i), err_pos=((T,), f), err_axis=((T,), f),
                    clearance=((T,), f), cand_theta=((T, R, nj), f), cand_status=((T, R), i), cand_iter=((T, R), i))

    def _mesh_table(self):
        return _args.mesh_table(self._meshes, self._D_mesh, 0 if self.mesh_variant is None else _lib.IK_MESH[self.mesh_variant])

    # ---- host arrays in and out (cfs_ik_solve) -----------------------------------------------------------------------------
    def solve(self, target_pos, target_axis=None, theta_ref=None, seed=0, want_candidates=False):
        """Solve T targets: target_pos (T, 3) or (3,); target_axis (T, 3), (3,) or None (position only); theta_ref (T, njoint),
        (njoint,) or None (the middle of the joint ranges).  Returns a namespace of numpy arrays, one row per target: theta
        (T, njoint), status (0 solved | 1 no restart converged | 2 every converged restart collides), selected (the winning restart,
        -1 without one), n_ok, err_pos, err_axis, clearance (min over the obstacles, meshes included, of distance - D; +inf without
        obstacles); rows
        of unsolved targets hold NaN.  want_candidates: also cand_theta (T, restarts, njoint), cand_status, cand_iter."""
        seed = _args.int_in(seed, "seed", 0, 2 ** 64 - 1)
        T, tp, ta, tr = self._targets(target_pos, target_axis, theta_ref)
        r = self._results(self._shapes(T), want_candidates)
        o = _args.fill(_lib.cfs_ik_out(), r)
        d = self._desc(ta is not None, seed, self.obs, self.D)
        if self._meshes:
            _lib.check(_lib.lib().cfs_ik_solve_mesh(C.byref(d), *self._mesh_table(), T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o)))
        else:
            _lib.check(_lib.lib().cfs_ik_solve(C.byref(d), T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o)))
        return r

    # ---- CUDA tensors in and out (cfs_ik_solve_device) ---------------------------------------------------------------------
    def solve_device(self, target_pos, target_axis=None, theta_ref=None, seed=0, want_candidates=False, stream=None):
        """solve() on float64 CUDA tensors of the solver's device (target_pos (T, 3), target_axis (T, 3) or None, theta_ref
        (T, njoint)), enqueued on `stream` (a torch.cuda.Stream; default: the current one) without a host synchronisation.  The
        values of device tensors cannot be checked on the host: a non-finite one ends the restarts that read it in state 3."""
        seed = _args.int_in(seed, "seed", 0, 2 ** 64 - 1)
        if torch is None:
            raise ValueError("solve_device needs torch")
        tp = _args.cuda_tensor(target_pos, "target_pos", (None, 3), device=self.device)
        T, dev = tp.shape[0], tp.device
        if T < 1:
            raise ValueError("at least one target is needed")
        ta = None if target_axis is None else _args.cuda_tensor(target_axis, "target_axis", (T, 3), device=dev)
        tr = self._theta_ref(theta_ref, T, dev)
        stream, obs, D = self._on(dev, stream)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            r = self._results(self._shapes(T), want_candidates, dev)
            o = _args.fill(_lib.cfs_ik_out(), r)
            d = self._desc(ta is not None, seed, obs, D)
            tail = (T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o), C.c_void_p(stream.cuda_stream))
            if self._meshes:
                _lib.check(_lib.lib().cfs_ik_solve_mesh_device(C.byref(d), *self._mesh_table(), *tail))
            else:
                _lib.check(_lib.lib().cfs_ik_solve_device(C.byref(d), *tail))
            self._record(stream, tp, ta, tr)
        return r
