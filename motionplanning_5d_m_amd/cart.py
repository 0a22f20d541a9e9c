"""Cartesian approach moves: batched straight-line tool paths over ``cfs_cart_path`` (include/cfs_hip.h, "Cartesian paths").

``IKSolver`` orients the tool at a goal; nothing moves it along the approach direction.  In a pick the free-space plan ends at a
pre-grasp pose a few centimetres back and the last stretch is a straight tool move into the grasp (a controller's LIN move; the
retreat is the same move in reverse).  ``CartesianPath`` traces that line from every configuration inverse kinematics found for the
pre-grasp (``cand_theta`` / ``cand_status``, accepted as they are) and keeps, per target, the candidate nearest to ``theta_ref`` whose
line completes inside the joint ranges, without a joint jump and free of the line obstacles.  One wavefront per target, one lane
per candidate; this module packs arguments and unpacks results, the tracing and the selection are a HIP kernel (csrc/cfs_cart.hip).

Mesh obstacles are opt-in: ``CartesianPath(..., meshes=True)`` takes an obs cell that ends with ``dict(mesh=Mesh, D=...)`` entries
and routes ``trace`` / ``trace_device`` to ``cfs_cart_path_mesh*`` (include/cfs_hip.h, "Cartesian paths against mesh obstacles";
DESIGN.md section 24): every accepted configuration of every line is also tested against the meshes with the decision of
``cfs_ik_solve_mesh``, and the clearance counts them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args, _lib
from ._args import f64 as _f64, ptr as _ptr
from .ik import _ToolSolver

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_CANDIDATES = 64          # one wavefront lane per candidate
MAX_STEPS = 256
MAX_ITER = 1000


class CartesianPath(_ToolSolver):
    """Straight tool lines for one robot, one set of line obstacles and one set of joint ranges.

    robot, obs, joint_limits, tool, tool_axis, tol_pos, tol_axis, weight, device, njoint: as for IKSolver, except that a mesh entry
    in `obs` is refused (line obstacles only) unless meshes=True.  steps: K line points after the start, 1..256.  max_iter:
    iterations per step, 1..1000.  max_joint_step (rad): the largest move of a joint between two line points; a larger one is a
    joint flip and ends the candidate.  meshes: False, or True for an obs cell that ends with mesh obstacles (dict(mesh=Mesh, D=...),
    D finite and > 0; at least one): a line then also ends, in state 2, at the first configuration whose link axes come closer to
    mesh j than max(D_j, 1e-4).  mesh_variant: as for IKSolver (None or "per_lane" | "wave" | "small_frontier", bit-identical
    results); needs meshes=True.  Arguments are validated here, before anything touches the device."""

    def __init__(self, robot, obs=None, joint_limits="robot", tool=None, tool_axis=None, steps=16, max_iter=20, max_joint_step=0.2,
                 tol_pos=1e-6, tol_axis=1e-6, weight=None, device=None, njoint=None, meshes=False, mesh_variant=None):
        obs = [] if obs is None else list(obs)
        if not isinstance(meshes, bool):
            raise ValueError(f"meshes must be True or False, not {meshes!r}")
        has_mesh = False
        for j, o in enumerate(obs):
            if isinstance(o, dict) and "mesh" in o:
                has_mesh = True
                if not meshes:
                    raise ValueError(f"obs[{j}] is a mesh obstacle: CartesianPath reads line obstacles only unless meshes=True")
        if meshes and not has_mesh:
            raise ValueError("meshes=True needs at least one mesh obstacle (dict(mesh=Mesh, D=...)) at the end of obs")
        if mesh_variant is not None and not meshes:
            raise ValueError("mesh_variant needs meshes=True")
        self.meshes = meshes
        self.mesh_variant = None if mesh_variant is None else _args.one_of(_lib.IK_MESH, mesh_variant, "mesh_variant")
        self.steps = _args.int_in(steps, "steps", 1, MAX_STEPS)
        self.max_iter = _args.int_in(max_iter, "max_iter", 1, MAX_ITER)
        super().__init__(robot, obs, joint_limits, tool, tool_axis, tol_pos, tol_axis, weight, device, njoint)
        self.max_joint_step = _args.real(max_joint_step, "max_joint_step")

    def _desc(self, use_axis, R, obs, D):
        d = self._fill_desc(_lib.cfs_cart_desc(), use_axis, obs, D)
        d.candidates, d.steps, d.max_iter, d.max_joint_step = int(R), self.steps, self.max_iter, self.max_joint_step
        return d

    def _mesh_table(self):
        return _args.mesh_table(self._meshes, self._D_mesh, 0 if self.mesh_variant is None else _lib.IK_MESH[self.mesh_variant])

    def _shapes(self, T, R, rows=None):
        """rows: the rows of a path (default: a straight line's steps + 1)"""
        nj, K1 = self.nj, self.steps + 1 if rows is None else rows
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
        return self._host(start, target_pos, target_axis, theta_ref, start_state, want_candidates, None)

    def _host(self, start, pos, axis, theta_ref, start_state, want_candidates, table):
        """trace (table None: pos / axis are target_pos / target_axis) and follow (table True: they are path_pos / path_axis): the
        arrays checked, the results allocated, one call of the host-array entry"""
        s = self._starts(start)
        if table is None:
            T, tp, ta, tr = self._targets(pos, axis, theta_ref)
            M, rows, entry, name = (), None, "cfs_cart_path", "target_pos"
        else:
            T, npts, tp, ta = self._table(pos, axis)
            tr = self._ref(theta_ref, T)
            M, rows, entry, name = (npts,), (npts - 1) * self.steps + 1, "cfs_cart_follow", "path_pos"
        if s.shape[0] != T:
            raise ValueError(f"start has {s.shape[0]} targets, {name} {T}")
        R = s.shape[1]
        ss = self._start_state(start_state, T, R)
        r = self._results(self._shapes(T, R, rows), want_candidates)
        o = _args.fill(_lib.cfs_cart_out(), r)
        d = self._desc(ta is not None, R, self.obs, self.D)
        tail = (T, *M, _ptr(s), _ptr(ss), _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o))
        mesh = self._mesh_table() if self.meshes else ()
        _lib.check(getattr(_lib.lib(), entry + ("_mesh" if self.meshes else ""))(C.byref(d), *mesh, *tail))
        return r

    def _starts(self, start):
        """the host array (T, R, nj) of the starts, validated (values are not: a bad start is state 5)"""
        nj = self.nj
        try:
            s = np.array(start, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"start must be an array of shape (T, R, {nj}) or (R, {nj})") from None
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or s.shape[2] != nj or s.shape[0] < 1 or not 1 <= s.shape[1] <= MAX_CANDIDATES:
            raise ValueError(f"start must have shape (T, R, {nj}) with T >= 1 and R in 1..{MAX_CANDIDATES}, not {s.shape}")
        return _f64(s)

    @staticmethod
    def _start_state(start_state, T, R):
        if start_state is None:
            return None
        try:
            ss = np.array(start_state)
        except (TypeError, ValueError):
            raise ValueError("start_state must be an integer array") from None
        if ss.ndim == 1:
            ss = ss[None]
        if ss.dtype.kind not in "iu" or ss.shape != (T, R):
            raise ValueError(f"start_state must be an integer array of shape ({T}, {R}), not {ss.dtype} {ss.shape}")
        return np.ascontiguousarray(ss.astype(np.int32))

    # ---- CUDA tensors in and out (cfs_cart_path_device) --------------------------------------------------------------------
    def trace_device(self, start, target_pos, target_axis=None, theta_ref=None, start_state=None, want_candidates=False, stream=None):
        """trace() on CUDA tensors of the solver's device: start (T, R, njoint), target_pos (T, 3), target_axis (T, 3) or None,
        theta_ref (T, njoint) or None float64; start_state (T, R) int32 or None; enqueued on `stream` (a torch.cuda.Stream; default:
        the current one) without a host synchronisation.  The values of device tensors cannot be checked on the host: a non-finite
        one ends the candidates that read it in state 3 (a start: state 5)."""
        if torch is None:
            raise ValueError("trace_device needs torch")
        return self._device(start, target_pos, target_axis, theta_ref, start_state, want_candidates, stream, None)

    def _device(self, start, pos, axis, theta_ref, start_state, want_candidates, stream, table):
        """trace_device (table None: pos / axis are target_pos / target_axis, (T, 3)) and follow_device (table True: they are
        path_pos / path_axis, (T, M, 3)): the tensors checked, the results and the cand_path workspace allocated, one launch on the
        stream, the tensors recorded on it"""
        nj = self.nj
        s = _args.cuda_tensor(start, "start", (None, None, nj), device=self.device)
        T, R, dev = s.shape[0], s.shape[1], s.device
        if T < 1 or not 1 <= R <= MAX_CANDIDATES:
            raise ValueError(f"start must have shape (T, R, {nj}) with T >= 1 and R in 1..{MAX_CANDIDATES}, not {tuple(s.shape)}")
        if table is None:
            M, rows, entry = (), None, "cfs_cart_path"
            tp = _args.cuda_tensor(pos, "target_pos", (T, 3), device=dev)
            ta = None if axis is None else _args.cuda_tensor(axis, "target_axis", (T, 3), device=dev)
        else:
            tp = _args.cuda_tensor(pos, "path_pos", (T, None, 3), device=dev)
            M, rows, entry = (self._npts(tp.shape[1]),), (tp.shape[1] - 1) * self.steps + 1, "cfs_cart_follow"
            ta = None if axis is None else _args.cuda_tensor(axis, "path_axis", (T, M[0], 3), device=dev)
        tr = self._theta_ref(theta_ref, T, dev)
        ss = None if start_state is None else _args.cuda_tensor(start_state, "start_state", (T, R), torch.int32, device=dev)
        stream, obs, D = self._on(dev, stream)
        shapes = self._shapes(T, R, rows)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            r = self._results(shapes, want_candidates, dev)
            o = _args.fill(_lib.cfs_cart_out(), r)
            work = None
            if not want_candidates:                           # `path` is gathered from cand_path: the launch's workspace
                work = _args.zeros_on(dev)(*shapes["cand_path"])
                o.cand_path = _ptr(work)
            d = self._desc(ta is not None, R, obs, D)
            tail = (T, *M, _ptr(s), _ptr(ss), _ptr(tp), _ptr(ta), _ptr(tr), C.byref(o), C.c_void_p(stream.cuda_stream))
            mesh = self._mesh_table() if self.meshes else ()
            _lib.check(getattr(_lib.lib(), entry + ("_mesh_device" if self.meshes else "_device"))(C.byref(d), *mesh, *tail))
            self._record(stream, s, ss, tp, ta, tr, work)
        return r

    # ---- polylines of tool poses (cfs_cart_follow*; include/cfs_hip.h, "Tool paths") -----------------------------------------
    def _npts(self, M):
        if not 2 <= M <= MAX_STEPS + 1:
            raise ValueError(f"path_pos must hold 2..{MAX_STEPS + 1} poses per target, not {M}")
        if (M - 1) * self.steps > MAX_STEPS:
            raise ValueError(f"(poses - 1) * steps = {(M - 1) * self.steps}: a path has at most {MAX_STEPS} rows after row 0")
        return int(M)

    def follow(self, start, path_pos, path_axis=None, theta_ref=None, start_state=None, want_candidates=False):
        """Follow T polylines of tool poses: path_pos (T, M, 3), or (M, 3) for one target, the points the tool passes in order;
        path_axis the same shape or None (position only), the tool direction at every point.  Consecutive poses are joined by
        straight moves of `steps` sub-steps each (the solver's steps, max_iter, max_joint_step, meshes= and mesh_variant= apply as
        they do to trace), so a path has N = (M-1)*steps + 1 rows, at most 257.  start, theta_ref, start_state: as for trace -- the
        candidates of an inverse-kinematics call at the first pose.  Unlike trace, row 0 is a pose to reach: a start that does not
        solve the first pose iterates towards it, and a start farther from its solution than max_joint_step is a joint jump.
        Returns trace's namespace with N rows in path and cand_path; theta is the winner's start."""
        return self._host(start, path_pos, path_axis, theta_ref, start_state, want_candidates, True)

    def _table(self, path_pos, path_axis):
        """the host arrays of the path tables, validated: (T, M, path_pos (T, M, 3), path_axis (T, M, 3) | None)"""
        try:
            pp = np.array(path_pos, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("path_pos must be an array of shape (T, M, 3) or (M, 3)") from None
        if pp.ndim == 2:
            pp = pp[None]
        if pp.ndim != 3 or pp.shape[2] != 3 or pp.shape[0] < 1:
            raise ValueError(f"path_pos must have shape (T, M, 3) with T >= 1 or (M, 3), not {pp.shape}")
        T, M = pp.shape[0], self._npts(pp.shape[1])
        if not np.isfinite(pp).all():
            raise ValueError("path_pos must be finite")
        pa = None
        if path_axis is not None:
            try:
                pa = np.array(path_axis, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("path_axis must be an array of the shape of path_pos, or None") from None
            if pa.ndim == 2:
                pa = pa[None]
            if pa.shape != (T, M, 3):
                raise ValueError(f"path_axis must have the shape of path_pos, ({T}, {M}, 3), not {pa.shape}")
            if not np.isfinite(pa).all():
                raise ValueError("path_axis must be finite")
            if not (np.linalg.norm(pa, axis=2) > 0).all():
                raise ValueError("a path_axis row is zero")
            pa = _f64(pa)
        return T, M, _f64(pp), pa

    def follow_device(self, start, path_pos, path_axis=None, theta_ref=None, start_state=None, want_candidates=False, stream=None):
        """follow() on CUDA tensors of the solver's device: start (T, R, njoint), path_pos (T, M, 3), path_axis (T, M, 3) or None,
        theta_ref (T, njoint) or None float64; start_state (T, R) int32 or None; enqueued on `stream` like trace_device, without a
        host synchronisation.  A non-finite value or a zero path_axis row ends the candidates that read it in state 3."""
        if torch is None:
            raise ValueError("follow_device needs torch")
        return self._device(start, path_pos, path_axis, theta_ref, start_state, want_candidates, stream, True)
