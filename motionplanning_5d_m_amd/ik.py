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
import math
import numbers
from types import SimpleNamespace

import numpy as np

from . import _lib
from .robotproperty2 import to_c_robot
from .mesh import Mesh
from .solvers import _f64, _joint_limits_array, _ptr, obs_meshes, obs_to_array

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_RESTARTS = 64            # one wavefront lane per restart
MAX_ITER = 1000


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _real(v, name, positive=True):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{name} must be a finite real number{' > 0' if positive else ''}, not {v!r}")
    return float(v)


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


class IKSolver:
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
        if not _is_int(restarts) or not 1 <= restarts <= MAX_RESTARTS:
            raise ValueError(f"restarts must be an integer in 1..{MAX_RESTARTS}, not {restarts!r}")
        if not _is_int(max_iter) or not 1 <= max_iter <= MAX_ITER:
            raise ValueError(f"max_iter must be an integer in 1..{MAX_ITER}, not {max_iter!r}")
        self.restarts, self.max_iter = int(restarts), int(max_iter)
        self.tol_pos, self.tol_axis = _real(tol_pos, "tol_pos"), _real(tol_axis, "tol_axis")
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
        self._meshes = obs_meshes(obs)                        # ValueError when a mesh precedes a line obstacle
        for j, o in enumerate(obs):
            if "mesh" not in o:
                continue
            if not isinstance(o["mesh"], Mesh):
                raise ValueError(f"obs[{j}]['mesh'] must be a Mesh, not {type(o['mesh']).__name__}")
            if isinstance(o.get("D"), bool) or not isinstance(o.get("D"), numbers.Real) or not math.isfinite(o["D"]) or not o["D"] > 0:
                raise ValueError(f"obs[{j}]['D'] (a mesh obstacle) must be a finite real number > 0")
        self._D_mesh = _f64([o["D"] for o in obs if "mesh" in o])
        if mesh_variant is not None and (not isinstance(mesh_variant, str) or mesh_variant not in _lib.IK_MESH):
            raise ValueError(f"mesh_variant must be None or one of {sorted(_lib.IK_MESH)}, not {mesh_variant!r}")
        self.mesh_variant = mesh_variant
        obs = [o for o in obs if "mesh" not in o]
        for j, o in enumerate(obs):
            if np.shape(o["l"]) != (3, 2) or not np.isfinite(np.asarray(o["l"], float)).all():
                raise ValueError(f"obs[{j}]['l'] must be a finite 3x2 array")
            if isinstance(o.get("D"), bool) or not isinstance(o.get("D"), numbers.Real) or not math.isfinite(o["D"]):
                raise ValueError(f"obs[{j}]['D'] must be a finite real number")
        self.obs = obs_to_array(obs) if obs else np.zeros((0, 6))
        self.D = _f64([o["D"] for o in obs])
        if device is not None:
            if torch is None:
                raise ValueError("device= needs torch")
            device = torch.device("cuda", int(device)) if _is_int(device) else torch.device(device)
            if device.type != "cuda":
                raise ValueError(f"device must be a CUDA (HIP) device, not {device}")
            if device.index is None:
                device = torch.device("cuda", 0)
        self.device = device
        self._dev = None                                      # obstacle rows on the device (solve_device)

    # ---- argument checks ---------------------------------------------------------------------------------------------------
    def _seed(self, seed):
        if not _is_int(seed) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in 0..2^64-1, not {seed!r}")
        return int(seed)

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
        return T, _f64(tp), (None if ta is None else _f64(ta)), _f64(tr)

    def _desc(self, use_axis, seed, obs, D):
        d = _lib.cfs_ik_desc()
        d.robot = to_c_robot(self.robot)
        d.njoint, d.use_axis = self.nj, int(use_axis)
        for q in range(3):
            d.tool[q], d.tool_axis[q] = float(self.tool[q]), float(self.tool_axis[q])
        d.lo, d.hi, d.weight = _ptr(self.lo), _ptr(self.hi), _ptr(self.weight)
        d.restarts, d.max_iter, d.tol_pos, d.tol_axis = self.restarts, self.max_iter, self.tol_pos, self.tol_axis
        d.nobs = int(self.obs.shape[0])
        d.obs, d.D = (_ptr(obs), _ptr(D)) if d.nobs else (None, None)
        d.seed = seed
        return d

    def _mesh_args(self):
        """(nmesh, handle array, D_mesh pointer, flags) of cfs_ik_solve_mesh*"""
        arr = (C.c_void_p * len(self._meshes))(*[m._h for m in self._meshes])
        return len(self._meshes), arr, _ptr(self._D_mesh), 0 if self.mesh_variant is None else _lib.IK_MESH[self.mesh_variant]

    # ---- host arrays in and out (cfs_ik_solve) -----------------------------------------------------------------------------
    def solve(self, target_pos, target_axis=None, theta_ref=None, seed=0, want_candidates=False):
        """Solve T targets: target_pos (T, 3) or (3,); target_axis (T, 3), (3,) or None (position only); theta_ref (T, njoint),
        (njoint,) or None (the middle of the joint ranges).  Returns a namespace of numpy arrays, one row per target: theta
        (T, njoint), status (0 solved | 1 no restart converged | 2 every converged restart collides), selected (the winning restart,
        -1 without one), n_ok, err_pos, err_axis, clearance (min over the obstacles, meshes included, of distance - D; +inf without
        obstacles); rows
        of unsolved targets hold NaN.  want_candidates: also cand_theta (T, restarts, njoint), cand_status, cand_iter."""
        seed = self._seed(seed)
        T, tp, ta, tr = self._targets(target_pos, target_axis, theta_ref)
        nj, R = self.nj, self.restarts
        r = SimpleNamespace(theta=np.zeros((T, nj)), status=np.zeros(T, np.int32), selected=np.zeros(T, np.int32), n_ok=np.zeros(T, np.int32),
                            err_pos=np.zeros(T), err_axis=np.zeros(T), clearance=np.zeros(T))
        if want_candidates:
            r.cand_theta, r.cand_status, r.cand_iter = np.zeros((T, R, nj)), np.zeros((T, R), np.int32), np.zeros((T, R), np.int32)
        o = _lib.cfs_ik_out()
        for k in vars(r):
            setattr(o, k, _ptr(getattr(r, k)))
        d = self._desc(ta is not None, seed, self.obs, self.D)
        if self._meshes:
            nm, arr, Dm, fl = self._mesh_args()
            _lib.check(_lib.lib().cfs_ik_solve_mesh(C.byref(d), nm, arr, Dm, fl, T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o)))
        else:
            _lib.check(_lib.lib().cfs_ik_solve(C.byref(d), T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o)))
        return r

    # ---- CUDA tensors in and out (cfs_ik_solve_device) ---------------------------------------------------------------------
    def solve_device(self, target_pos, target_axis=None, theta_ref=None, seed=0, want_candidates=False, stream=None):
        """solve() on float64 CUDA tensors of the solver's device (target_pos (T, 3), target_axis (T, 3) or None, theta_ref
        (T, njoint)), enqueued on `stream` (a torch.cuda.Stream; default: the current one) without a host synchronisation.  The
        values of device tensors cannot be checked on the host: a non-finite one ends the restarts that read it in state 3."""
        seed = self._seed(seed)
        if torch is None:
            raise ValueError("solve_device needs torch")
        nj, R = self.nj, self.restarts

        def chk(t, name, cols):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 CUDA tensor")
            if t.ndim != 2 or t.shape[1] != cols:
                raise ValueError(f"{name} must have shape (T, {cols}), not {tuple(t.shape)}")
            if self.device is not None and t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the solver on {self.device}")
            return t.contiguous()
        tp = chk(target_pos, "target_pos", 3)
        T, dev = tp.shape[0], tp.device
        if T < 1:
            raise ValueError("at least one target is needed")
        ta = None if target_axis is None else chk(target_axis, "target_axis", 3)
        if theta_ref is None:
            tr = torch.tensor(0.5 * (self.lo + self.hi), dtype=torch.float64, device=dev).unsqueeze(0).expand(T, -1).contiguous()
        else:
            tr = chk(theta_ref, "theta_ref", nj)
        for t, name in ((ta, "target_axis"), (tr, "theta_ref")):
            if t is not None and (t.shape[0] != T or t.device != dev):
                raise ValueError(f"{name} must have {T} rows on {dev}")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        elif not isinstance(stream, torch.cuda.Stream):
            raise ValueError("stream must be a torch.cuda.Stream")
        if self._dev is None or self._dev[0] != dev:
            self._dev = (dev, torch.tensor(self.obs, dtype=torch.float64, device=dev), torch.tensor(self.D, dtype=torch.float64, device=dev))
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            z = lambda *sh, dt=torch.float64: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
            r = SimpleNamespace(theta=z(T, nj), status=z(T, dt=torch.int32), selected=z(T, dt=torch.int32), n_ok=z(T, dt=torch.int32),
                                err_pos=z(T), err_axis=z(T), clearance=z(T))
            if want_candidates:
                r.cand_theta, r.cand_status, r.cand_iter = z(T, R, nj), z(T, R, dt=torch.int32), z(T, R, dt=torch.int32)
            o = _lib.cfs_ik_out()
            for k in vars(r):
                setattr(o, k, _ptr(getattr(r, k)))
            d = self._desc(ta is not None, seed, self._dev[1], self._dev[2])
            if self._meshes:
                nm, arr, Dm, fl = self._mesh_args()
                _lib.check(_lib.lib().cfs_ik_solve_mesh_device(C.byref(d), nm, arr, Dm, fl, T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o),
                                                               C.c_void_p(stream.cuda_stream)))
            else:
                _lib.check(_lib.lib().cfs_ik_solve_device(C.byref(d), T, _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o), C.c_void_p(stream.cuda_stream)))
            for t in (tp, ta, tr, self._dev[1], self._dev[2]):
                if t is not None:
                    t.record_stream(stream)
        return r
