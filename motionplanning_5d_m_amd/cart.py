"""Cartesian approach moves: batched straight-line tool paths over ``cfs_cart_path`` (include/cfs_hip.h, "Cartesian paths").

``IKSolver`` orients the tool at a goal; nothing moves it along the approach direction.  In a pick the free-space plan ends at a
pre-grasp pose a few centimetres back and the last stretch is a straight tool move into the grasp (a controller's LIN move; the
retreat is the same move in reverse).  ``CartesianPath`` traces that line from every configuration inverse kinematics found for the
pre-grasp (``cand_theta`` / ``cand_status``, accepted as they are) and keeps, per target, the candidate nearest to ``theta_ref`` whose
line completes inside the joint ranges, without a joint jump and free of the line obstacles.  One wavefront per target, one lane
per candidate; this module packs arguments and unpacks results, the tracing and the selection are a HIP kernel (csrc/cfs_cart.hip).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib
from .ik import IKSolver, _is_int, _real
from .robotproperty2 import to_c_robot
from .solvers import _f64, _ptr

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_CANDIDATES = 64          # one wavefront lane per candidate
MAX_STEPS = 256
MAX_ITER = 1000


class CartesianPath:
    """Straight tool lines for one robot, one set of line obstacles and one set of joint ranges.

    robot, obs, joint_limits, tool, tool_axis, tol_pos, tol_axis, weight, device, njoint: as for IKSolver, except that a mesh entry
    in `obs` is refused (line obstacles only).  steps: K line points after the start, 1..256.  max_iter: iterations per step,
    1..1000.  max_joint_step (rad): the largest move of a joint between two line points; a larger one is a joint flip and ends the
    candidate.  Arguments are validated here, before anything touches the device."""

    def __init__(self, robot, obs=None, joint_limits="robot", tool=None, tool_axis=None, steps=16, max_iter=20, max_joint_step=0.2,
                 tol_pos=1e-6, tol_axis=1e-6, weight=None, device=None, njoint=None):
        obs = [] if obs is None else list(obs)
        for j, o in enumerate(obs):
            if isinstance(o, dict) and "mesh" in o:
                raise ValueError(f"obs[{j}] is a mesh obstacle: CartesianPath reads line obstacles only")
        if not _is_int(steps) or not 1 <= steps <= MAX_STEPS:
            raise ValueError(f"steps must be an integer in 1..{MAX_STEPS}, not {steps!r}")
        if not _is_int(max_iter) or not 1 <= max_iter <= MAX_ITER:
            raise ValueError(f"max_iter must be an integer in 1..{MAX_ITER}, not {max_iter!r}")
        # the shared arguments are IKSolver's, checked by IKSolver's own code
        base = IKSolver(robot, obs, joint_limits=joint_limits, tool=tool, tool_axis=tool_axis, restarts=1, max_iter=int(max_iter),
                        tol_pos=tol_pos, tol_axis=tol_axis, weight=weight, device=device, njoint=njoint)
        self.robot, self.nj, self.lo, self.hi = base.robot, base.nj, base.lo, base.hi
        self.tool, self.tool_axis, self.weight = base.tool, base.tool_axis, base.weight
        self.tol_pos, self.tol_axis, self.obs, self.D, self.device = base.tol_pos, base.tol_axis, base.obs, base.D, base.device
        self._targets = base._targets
        self.steps, self.max_iter = int(steps), int(max_iter)
        self.max_joint_step = _real(max_joint_step, "max_joint_step")
        self._dev = None                                      # obstacle rows on the device (trace_device)

    def _desc(self, use_axis, R, obs, D):
        d = _lib.cfs_cart_desc()
        d.robot = to_c_robot(self.robot)
        d.njoint, d.use_axis = self.nj, int(use_axis)
        for q in range(3):
            d.tool[q], d.tool_axis[q] = float(self.tool[q]), float(self.tool_axis[q])
        d.lo, d.hi, d.weight = _ptr(self.lo), _ptr(self.hi), _ptr(self.weight)
        d.candidates, d.steps, d.max_iter, d.max_joint_step = int(R), self.steps, self.max_iter, self.max_joint_step
        d.tol_pos, d.tol_axis = self.tol_pos, self.tol_axis
        d.nobs = int(self.obs.shape[0])
        d.obs, d.D = (_ptr(obs), _ptr(D)) if d.nobs else (None, None)
        return d

    def _names(self, want_candidates):
        return ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance") + (
            ("cand_status", "cand_done", "cand_iter", "cand_end", "cand_path") if want_candidates else ())

    def _shapes(self, T, R):
        nj, K1 = self.nj, self.steps + 1
        f, i = np.float64, np.int32
        return dict(theta=((T, nj), f), status=((T,), i), path=((T, K1, nj), f), selected=((T,), i), n_ok=((T,), i), n_done=((T,), i),
                    clearance=((T,), f), cand_status=((T, R), i), cand_done=((T, R), i), cand_iter=((T, R), i), cand_end=((T, R, nj), f),
                    cand_path=((T, R, K1, nj), f))

    # ---- host arrays in and out (cfs_cart_path) ----------------------------------------------------------------------------
    def trace(self, start, target_pos, target_axis=None, theta_ref=None, start_state=None, want_candidates=False):
        """Trace T targets: start (T, R, njoint) or (R, njoint) for one target -- IKSolver's cand_theta, NaN and out-of-range rows
        allowed (such a candidate has no start) --; target_pos (T, 3) or (3,); target_axis (T, 3), (3,) or None (position only);
        theta_ref (T, njoint), (njoint,) or None (the middle of the joint ranges); start_state (T, R) integers or None (every start
        is used): IKSolver's cand_status, a candidate runs only when its entry is 0.  Returns a namespace of numpy arrays, one row
        per target: theta (T, njoint; the winner's start), status (0 solved | 1 some candidate had a start but none completed | 2
        no candidate had a start), path (T, steps+1, njoint), selected (-1 without a winner), n_ok, n_done, clearance (the minimum
        over the path's configurations); rows of unsolved targets hold NaN.  want_candidates: also cand_status (0 complete | 1 a
        step did not converge | 2 collision | 3 numeric | 4 joint jump | 5 no start), cand_done, cand_iter (T, R), cand_end
        (T, R, njoint) and cand_path (T, R, steps+1, njoint; NaN after cand_done)."""
        nj = self.nj
        try:
            s = np.array(start, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"start must be an array of shape (T, R, {nj}) or (R, {nj})") from None
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or s.shape[2] != nj or s.shape[0] < 1 or not 1 <= s.shape[1] <= MAX_CANDIDATES:
            raise ValueError(f"start must have shape (T, R, {nj}) with T >= 1 and R in 1..{MAX_CANDIDATES}, not {s.shape}")
        T, tp, ta, tr = self._targets(target_pos, target_axis, theta_ref)
        if s.shape[0] != T:
            raise ValueError(f"start has {s.shape[0]} targets, target_pos {T}")
        R = s.shape[1]
        ss = None
        if start_state is not None:
            try:
                ss = np.array(start_state)
            except (TypeError, ValueError):
                raise ValueError("start_state must be an integer array") from None
            if ss.ndim == 1:
                ss = ss[None]
            if ss.dtype.kind not in "iu" or ss.shape != (T, R):
                raise ValueError(f"start_state must be an integer array of shape ({T}, {R}), not {ss.dtype} {ss.shape}")
            ss = np.ascontiguousarray(ss.astype(np.int32))
        s = _f64(s)
        shapes = self._shapes(T, R)
        r = SimpleNamespace(**{k: np.zeros(*shapes[k]) for k in self._names(want_candidates)})
        o = _lib.cfs_cart_out()
        for k in vars(r):
            setattr(o, k, _ptr(getattr(r, k)))
        d = self._desc(ta is not None, R, self.obs, self.D)
        _lib.check(_lib.lib().cfs_cart_path(C.byref(d), T, _ptr(s), _ptr(ss), _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o)))
        return r

    # ---- CUDA tensors in and out (cfs_cart_path_device) --------------------------------------------------------------------
    def trace_device(self, start, target_pos, target_axis=None, theta_ref=None, start_state=None, want_candidates=False, stream=None):
        """trace() on CUDA tensors of the solver's device: start (T, R, njoint), target_pos (T, 3), target_axis (T, 3) or None,
        theta_ref (T, njoint) or None float64; start_state (T, R) int32 or None; enqueued on `stream` (a torch.cuda.Stream; default:
        the current one) without a host synchronisation.  The values of device tensors cannot be checked on the host: a non-finite
        one ends the candidates that read it in state 3 (a start: state 5)."""
        if torch is None:
            raise ValueError("trace_device needs torch")
        nj = self.nj

        def chk(t, name, shape, dtype=None):
            dtype = torch.float64 if dtype is None else dtype
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
                raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} CUDA tensor")
            if t.ndim != len(shape) or any(w is not None and v != w for v, w in zip(t.shape, shape)):
                raise ValueError(f"{name} must have shape {tuple('T' if w is None else w for w in shape)}, not {tuple(t.shape)}")
            if self.device is not None and t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the solver on {self.device}")
            return t.contiguous()
        s = chk(start, "start", (None, None, nj))
        T, R, dev = s.shape[0], s.shape[1], s.device
        if T < 1 or not 1 <= R <= MAX_CANDIDATES:
            raise ValueError(f"start must have shape (T, R, {nj}) with T >= 1 and R in 1..{MAX_CANDIDATES}, not {tuple(s.shape)}")
        tp = chk(target_pos, "target_pos", (T, 3))
        ta = None if target_axis is None else chk(target_axis, "target_axis", (T, 3))
        if theta_ref is None:
            tr = torch.tensor(0.5 * (self.lo + self.hi), dtype=torch.float64, device=dev).unsqueeze(0).expand(T, -1).contiguous()
        else:
            tr = chk(theta_ref, "theta_ref", (T, nj))
        ss = None if start_state is None else chk(start_state, "start_state", (T, R), torch.int32)
        for t, name in ((tp, "target_pos"), (ta, "target_axis"), (tr, "theta_ref"), (ss, "start_state")):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} must be on {dev}")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        elif not isinstance(stream, torch.cuda.Stream):
            raise ValueError("stream must be a torch.cuda.Stream")
        if self._dev is None or self._dev[0] != dev:
            self._dev = (dev, torch.tensor(self.obs, dtype=torch.float64, device=dev), torch.tensor(self.D, dtype=torch.float64, device=dev))
        shapes = self._shapes(T, R)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            z = lambda k: torch.zeros(*shapes[k][0], dtype=torch.float64 if shapes[k][1] is np.float64 else torch.int32, device=dev)  # noqa: E731
            r = SimpleNamespace(**{k: z(k) for k in self._names(want_candidates)})
            o = _lib.cfs_cart_out()
            for k in vars(r):
                setattr(o, k, _ptr(getattr(r, k)))
            work = None
            if not want_candidates:                           # `path` is gathered from cand_path: the launch's workspace
                work = z("cand_path")
                o.cand_path = _ptr(work)
            d = self._desc(ta is not None, R, self._dev[1], self._dev[2])
            _lib.check(_lib.lib().cfs_cart_path_device(C.byref(d), T, _ptr(s), _ptr(ss), _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o),
                                                       C.c_void_p(stream.cuda_stream)))
            for t in (s, ss, tp, ta, tr, work, self._dev[1], self._dev[2]):
                if t is not None:
                    t.record_stream(stream)
        return r
