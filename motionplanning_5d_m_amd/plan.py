"""RRTstar_CFS.m as one batched pipeline: K RRT seeds per slot, every route smoothed, the best smoothed result kept.

The reference plans one start/goal pair (RRTstar_CFS.m): rounds of ``num_seed`` RRT seeds until one succeeds
(Lib/functions/s_Parallel_rrt.m:14-28), the route with the fewest nodes (:27-28), one CFS on it (RRTstar_CFS.m:94-196).
``RRTCFSPlanner.plan`` does that for S slots at once, entirely on the GPU:

* grow   -- S*K trees in one ``cfs_rrt_grow_device`` launch (``cfs_rrt_grow_mesh_device`` in a cell with mesh obstacles); slots
            none of whose seeds found a route are regrown, alone, in the next round (the reference's ``while all(path_fail)``);
* build  -- one ``cfs_build_terms_from_ragged_routes_device`` call (cubic resampling to H+1 = 41 points + cost terms);
* solve  -- one ``cfs_solve_batch_device`` over all S*K candidates (select="best") or over the S shortest routes
            (select="shortest", the reference's rule);
* audit  -- optional (min_clearance=): one ``cfs_clearance_device`` launch measures every smoothed candidate along the motion
            between its waypoints; a candidate that comes closer to an obstacle than margin - slack is not eligible;
* select -- ``cfs_select_best_device``: per slot the best smoothed candidate by the rule of include/cfs_hip.h.

This module packs arguments, indexes tensors (placeholder routes, the shortest route's index for select="shortest") and reads
S fail flags per round; tree growth, resampling, the solves and the selection are HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from types import SimpleNamespace

import numpy as np

from . import _args, _lib
from ._args import ptr as _ptr
from .cart import MAX_STEPS, CartesianPath
from .ik import IKSolver
from .rrt import RRT_FANUC
from .timing import MAX_ROWS, MIN_ROWS, PathTimer
from .audit import MAX_SUBSTEPS, PathAudit
from .robotproperty2 import robotproperty2
from .solvers import SOLVE_OUT, CFSBatch, _infeasible_args, _joint_limits_array, obs_meshes, obs_to_array
from .sysinfo import RRTstar_CFS_problem

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SELECT = ("best", "shortest")
MAX_SEEDS = 64               # one wavefront lane per candidate in cfs_select_best_device
ROUND_SEED_STRIDE = 1_000_003  # R: the trees of round r use the generator seed `seed + r*R`


def select_best_device(cfs, S, K, route_ok, cand, best, selected, has_solution, cand_viol_all=None, best_viol_all=None, stream=None):
    """cfs_select_best_device on CUDA tensors: cand / best are CFSBatch.alloc_outputs-style namespaces of S*K / S rows,
    route_ok (S*K,) int32, selected / has_solution (S,) int32, viol_all (rows, MAX_O_ITER) float64 or None."""
    stream = _args.stream_ptr(stream, route_ok.device)
    cand, best = _args.fill(_lib.cfs_batch_out(), cand), _args.fill(_lib.cfs_batch_out(), best)
    _lib.check(cfs._lib.cfs_select_best_device(cfs._h, int(S), int(K), _ptr(route_ok), C.byref(cand), _ptr(cand_viol_all), C.byref(best),
                                               _ptr(best_viol_all), _ptr(selected), _ptr(has_solution), C.c_void_p(stream)))


class RRTCFSPlanner:
    """RRTstar_CFS.m's pipeline for up to max_slots (start, goal) slots per call, num_seed RRT seeds per slot.

    select="best": every seed's route is smoothed and the best smoothed result per slot is kept (cfs_select_best_device:
    status 0/1 by lowest final cost, else status 4 by lowest final violation then cost).  select="shortest": the reference's
    rule -- the route with the fewest nodes, first seed on ties (s_Parallel_rrt.m:27-28) -- then one CFS per slot.
    The cost family is RRTstar_CFS.m:124-187's (sysinfo.RRTstar_CFS_problem: M200i, H = 40); the obstacles are `pobs`, with
    margins obs{j}.epsilon (CFS) or obs{j}.D (PSGCFS).  joint_limits: None | "robot" | a (5, 2) array of [lo, hi], the smoothing
    QPs' position rows (CFSBatch; the RRT samples ignore them).
    min_clearance: None (the default: no audit, results exactly those without the argument) | slack in metres (>= 0): after the
    solve every candidate is audited with audit_substeps samples per interval (CFSBatch.clearance_device) and is eligible only if
    dist_path[j] >= margin_j - slack for every obstacle j.  A slot none of whose found routes passes keeps the candidate the
    plain rule names, with has_solution = 0.  Results then carry dist_path, dist_lower (S, nobs) and clearance_ok (S).
    Mesh obstacles: `pobs` may end with dict(mesh=Mesh, D=..., epsilon=...) entries (after the line obstacles, as for CFS_FANUC):
    the trees then grow around the meshes (cfs_rrt_grow_mesh_device), the smoothing handle measures them (set_meshes; their rows of
    the obs tensor are zero) and min_clearance audits with clearance_mesh_device.  What the handle refuses is refused here: meshes
    with on_infeasible="soften", a mesh before a line obstacle, a mesh margin that is not finite and > 0.  Without meshes the
    planner is exactly the line-obstacle one.
    Arguments are validated before anything touches the device."""

    def __init__(self, pobs, sys_rrt, region_g, region_s, sample_off, ROBOT="M200i", rrt_solver="RRT", num_seed=6, mode="CFS",
                 select="best", on_infeasible="stop", soft_weight=None, jacobian="fd_literal", max_slots=256, device=None,
                 joint_limits=None, min_clearance=None, audit_substeps=16):
        _args.one_of(SELECT, select, "select")
        _args.int_in(num_seed, "num_seed", 1, MAX_SEEDS)
        _args.int_in(max_slots, "max_slots", 1)
        _args.one_of(_lib.MODE, mode, "mode")
        if rrt_solver not in ("RRT", "RRT*"):
            raise ValueError(f"rrt_solver must be 'RRT' or 'RRT*', not {rrt_solver!r}")
        if ROBOT != "M200i":
            raise ValueError(f"the cost family is RRTstar_CFS.m's (M200i); ROBOT={ROBOT!r} is not supported")
        if int(getattr(sys_rrt, "nstate", 0)) != 5:
            raise ValueError("sys_rrt.nstate must be 5 (the M200i's joints)")
        _args.code(_lib.JACOBIAN, jacobian, "jacobian")
        _infeasible_args(on_infeasible, soft_weight)
        lim = _joint_limits_array(joint_limits, robotproperty2("M200i"), 5)
        self._ik_limits = lim if lim is not None else "robot"                       # plan_to_pose: the planner's ranges, else robot.thetamax
        self._pobs, self._sys_rrt, self._ik = list(pobs), sys_rrt, {}
        meshes = obs_meshes(pobs)                                                   # ValueError: a mesh before a line obstacle
        if meshes and on_infeasible == "soften":
            raise ValueError('on_infeasible="soften" does not support mesh obstacles')
        for o in pobs:
            if "mesh" in o and not all(isinstance(o.get(k), numbers.Real) and math.isfinite(o[k]) and o[k] > 0 for k in ("D", "epsilon")):
                raise ValueError("a mesh obstacle needs finite D and epsilon > 0")
        if min_clearance is not None and _args.real(min_clearance, "min_clearance", positive=False) < 0:
            raise ValueError(f"min_clearance must be None or a finite slack >= 0 in metres, not {min_clearance!r}")
        self.min_clearance = None if min_clearance is None else float(min_clearance)
        self.audit_substeps = _args.int_in(audit_substeps, "audit_substeps", 1, 64)
        if device is None:                                                          # torch's current device
            device = torch.cuda.current_device() if torch is not None and torch.cuda.is_available() else 0
        device = _args.cuda_device(device)
        self.select, self.K, self.max_slots, self.mode = select, int(num_seed), int(max_slots), mode
        self.on_infeasible, self.device, self.nj = on_infeasible, device, 5
        self.rrt = RRT_FANUC(pobs, sys_rrt, sys_rrt.goal_th, region_g, region_s, sample_off, ROBOT, rrt_solver)
        self.N = RRT_FANUC.MAX_ITER + 1
        _, self.sys_cfs, _ = RRTstar_CFS_problem(np.stack([np.asarray(sys_rrt.x0, float), np.asarray(sys_rrt.goal_th, float)], axis=1))
        margin = [o["epsilon"] if mode == "CFS" else o["D"] for o in pobs]
        self.cfs = CFSBatch(self.sys_cfs, len(pobs), margin, mode=mode, max_batch=self.max_slots * self.K, device=device.index,
                            jacobian=jacobian, on_infeasible=on_infeasible, soft_weight=soft_weight, joint_limits=joint_limits)
        one = torch.tensor(obs_to_array(pobs), dtype=torch.float64, device=device)
        self._obs = one.unsqueeze(0).expand(self.max_slots * self.K, -1, -1).contiguous()
        self._meshes = meshes
        if meshes:
            self.cfs.set_meshes(meshes)

    def close(self):
        self.cfs.close()

    # ---- argument checks (no GPU call before they pass) --------------------------------------------------------------------
    def _conv(self, v, name, cols, nonzero=False, table=False):
        """v as a float64 tensor (given a tensor on the planner's device) or a finite numpy array (goes to the device once validated)
        of shape (cols,) or (S, cols) -- table: (M, cols) or (S, M, cols), M rows per slot --; nonzero: no row of an array may be zero"""
        dims = (2, 3) if table else (1, 2)
        if torch is not None and isinstance(v, torch.Tensor):
            if v.device != self.device:
                raise ValueError(f"{name} is on {v.device}, the planner on {self.device}")
            if not v.dtype.is_floating_point:
                raise ValueError(f"{name} must be a floating-point tensor, not {v.dtype}")
            t = v.to(torch.float64)
        else:
            try:
                t = np.array(v, dtype=float)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be numeric") from None
            if not np.isfinite(t).all():
                raise ValueError(f"{name} must be finite")
            if nonzero and t.ndim in dims and t.shape[-1] == cols and not (np.linalg.norm(t.reshape(-1, cols), axis=1) > 0).all():
                raise ValueError(f"a {name} row is zero")
        if t.ndim not in dims or t.shape[-1] != cols:
            want = f"(M, {cols}) or (S, M, {cols})" if table else f"({cols},) or (S, {cols})"
            raise ValueError(f"{name} must have shape {want}, not {tuple(t.shape)}")
        return t

    def _pair(self, x0, goal):
        x0, goal = self._conv(x0, "x0", self.nj), self._conv(goal, "goal", self.nj)
        S = max(x0.shape[0] if x0.ndim == 2 else 1, goal.shape[0] if goal.ndim == 2 else 1)
        for t, name in ((x0, "x0"), (goal, "goal")):
            if t.ndim == 2 and t.shape[0] != S:
                raise ValueError(f"x0 and goal disagree on S: {tuple(x0.shape)} vs {tuple(goal.shape)}")
        if S < 1 or S > self.max_slots:
            raise ValueError(f"S={S} outside 1..max_slots={self.max_slots}")
        return S, x0, goal

    def _on_device(self, t, S):
        if not (torch is not None and isinstance(t, torch.Tensor)):
            t = torch.tensor(t, dtype=torch.float64, device=self.device)
        if t.ndim == 1:
            t = t.unsqueeze(0).expand(S, -1)
        return t.contiguous()

    # ---- Cartesian goals ---------------------------------------------------------------------------------------------------
    def plan_to_pose(self, x0, target_pos, target_axis=None, seed=0, ik_options=None, ik_meshes=False, approach=None, approach_dir=None,
                     approach_steps=16, approach_options=None, approach_meshes=False, approach_timing=None, approach_audit=None, **plan_kwargs):
        """plan() towards Cartesian targets: one inverse-kinematics launch (ik.IKSolver.solve_device: theta_ref = x0, the planner's
        obstacles with their D -- its line obstacles, and with ik_meshes=True its mesh obstacles too --, the planner's joint_limits if
        it has them, else robot.thetamax; generator seed `seed`), then
        plan(x0, goal, seed, **plan_kwargs) with the configurations it found.  x0: (S, 5) or (5,); target_pos: (S, 3) or (3,):
        where the tool point goes (default tool: the reference's end effector cap{5}.p(:,1)); target_axis: (S, 3), (3,) or None
        (position only): where the tool axis points.  CUDA tensors on the planner's device or array-likes.  ik_options: keyword
        arguments of IKSolver (tool, tool_axis, restarts, max_iter, tol_pos, tol_axis, weight).
        Returns plan()'s namespace plus goal (S, 5; NaN rows without an IK solution), ik_status (0 solved | 1 no restart converged
        | 2 every converged restart collides), ik_err_pos, ik_clearance.  A slot without an IK solution is planned with goal = x0
        (the batch keeps its shape) and then masked: status = -2, has_solution = 0, selected = -1.
        ik_meshes: False (the default) keeps the line-only IK collision test, and a planner with mesh obstacles then refuses;
        True builds the solver from the planner's whole cell -- the lines with their D and the meshes with their D, the numbers
        cfs_rrt_grow_mesh_device gets -- so that goals are free of the meshes too (cfs_ik_solve_mesh_device).  On a planner without
        meshes ik_meshes=True is the default path.
        approach: None (the default: everything above, bit for bit) or a distance > 0 in metres, a number or (S,): the plan then ends
        at a pre-grasp pose `approach` metres back from target_pos and the tool enters the grasp along a straight line
        (cart.CartesianPath; needs target_axis; on a planner with mesh obstacles it needs approach_meshes=True).  approach_dir:
        (S, 3), (3,) or None (= target_axis): the world direction the tool travels on that line.  One IK launch at
        target_pos - approach*unit(dir) with its candidates kept, one trace_device launch from every candidate (cand_theta / cand_status) to target_pos on the same stream
        (approach_steps line points; approach_options: CartesianPath's max_iter, max_joint_step; tool, tolerances and weight are
        ik_options'), then plan() with the winners' starts as goals: per slot the IK candidate nearest to x0 whose line completes.
        The result gains approach_path (S, approach_steps+1, 5), grasp (= approach_path[:, -1]), approach_status (CartesianPath's
        status), approach_clearance, approach_selected and ik_goal (IK's own winner); goal is the configuration planned to.  A slot
        whose IK solved but whose approach did not gets status = -3 and is masked like -2.
        approach_meshes: False (the default) keeps the line-only trace, and a planner with mesh obstacles then refuses an approach;
        True (needs ik_meshes=True on such a planner) builds the CartesianPath from the planner's whole cell with meshes=True -- the
        D that cfs_rrt_grow_mesh_device gets --, so that every configuration of the line is free of the meshes too
        (cfs_cart_path_mesh_device).  On a planner without meshes it is the line-only path.
        approach_timing: None (the default: everything above, bit for bit) or a dict of timing.PathTimer's vmax, amax (both needed),
        feed, stops, curve_share: the winners' approach paths are then timed on the same stream (stops="corners" reads
        approach_steps), and the result gains approach_time, approach_sdot (S, approach_steps+1), approach_duration and
        approach_time_status (PathTimer's status; a slot without an approach path: NaN rows and status 1).  Needs approach and
        approach_steps >= 2.
        approach_audit: None (the default: everything above, bit for bit) or a dict of substeps (default 8), min_clearance, max_chord
        (audit.PathAudit's; a missing one is not tested): the line is then traced with every candidate kept, all of them are audited
        between their rows on the same stream, and per slot the candidate nearest to x0 that passes is taken, as plan_to_path's
        path_audit takes it: status -4 for a slot with a complete line none of which passes, and the result gains
        approach_clear_lower, approach_clear_path, approach_chord_err, approach_chord_upper and approach_audit_state.  Needs approach;
        a planner with meshes refuses."""
        if approach_audit is not None and self._meshes:
            raise ValueError("approach_audit on a planner with mesh obstacles: meshes are not audited between the rows (line obstacles only)")
        if approach is None:
            if approach_dir is not None or approach_options is not None or approach_timing is not None or approach_audit is not None:
                raise ValueError("approach_dir / approach_options / approach_timing / approach_audit need approach")
        else:
            if self._meshes and approach_meshes is not True:
                raise ValueError("plan_to_pose(approach=...) on a planner with mesh obstacles: the straight-line trace reads line obstacles only "
                                 "unless approach_meshes=True")
            if target_axis is None:
                raise ValueError("approach needs target_axis: the tool keeps its direction along the line")
            if approach_options is None:
                approach_options = {}
            if not isinstance(approach_options, dict) or set(approach_options) - {"max_iter", "max_joint_step"}:
                raise ValueError("approach_options must be a dict of CartesianPath's max_iter, max_joint_step")
        _args.int_in(approach_steps, "approach_steps", 1, MAX_STEPS)
        if not isinstance(ik_meshes, bool):
            raise ValueError(f"ik_meshes must be True or False, not {ik_meshes!r}")
        if not isinstance(approach_meshes, bool):
            raise ValueError(f"approach_meshes must be True or False, not {approach_meshes!r}")
        if approach_meshes and approach is None:
            raise ValueError("approach_meshes needs approach")
        if self._meshes and not ik_meshes:
            raise ValueError("plan_to_pose on a planner with mesh obstacles needs ik_meshes=True: the default IK collision test reads "
                             "line obstacles only")
        _args.int_in(seed, "seed", 0)
        if ik_options is None:
            ik_options = {}
        if not isinstance(ik_options, dict) or set(ik_options) - {"tool", "tool_axis", "restarts", "max_iter", "tol_pos", "tol_axis", "weight"}:
            raise ValueError("ik_options must be a dict of IKSolver's tool, tool_axis, restarts, max_iter, tol_pos, tol_axis, weight")
        stream = plan_kwargs.get("stream")
        if stream is not None:
            _args.as_stream(stream, self.device)
        args = [self._conv(x0, "x0", self.nj), self._conv(target_pos, "target_pos", 3)]
        if target_axis is not None:
            args.append(self._conv(target_axis, "target_axis", 3, nonzero=True))
        adir = dist = None
        if approach is not None:
            adir = args[2] if approach_dir is None else self._conv(approach_dir, "approach_dir", 3, nonzero=True)
            if torch is not None and isinstance(approach, torch.Tensor):
                if approach.device != self.device or not approach.dtype.is_floating_point or approach.ndim > 1:
                    raise ValueError(f"approach must be a floating-point tensor of shape () or (S,) on {self.device}")
                dist = approach.to(torch.float64)
            else:
                if isinstance(approach, (bool, str)):
                    raise ValueError(f"approach must be a distance > 0 or (S,) distances, not {approach!r}")
                try:
                    dist = np.array(approach, dtype=float)
                except (TypeError, ValueError):
                    raise ValueError(f"approach must be a distance > 0 or (S,) distances, not {approach!r}") from None
                if dist.ndim > 1 or not np.isfinite(dist).all() or not (dist > 0).all():
                    raise ValueError(f"approach must be a finite distance > 0 or (S,) of them, not {approach!r}")
        rows = {a.shape[0] for a in args + ([adir] if adir is not None else []) if a.ndim == 2}
        if dist is not None and dist.ndim == 1:
            rows.add(dist.shape[0])
        if len(rows) > 1:
            raise ValueError(f"x0, target_pos, target_axis, approach and approach_dir disagree on S: {sorted(rows)}")
        S = rows.pop() if rows else 1
        if S < 1 or S > self.max_slots:
            raise ValueError(f"S={S} outside 1..max_slots={self.max_slots}")
        key = tuple(sorted((k, repr(v)) for k, v in ik_options.items()))
        if key not in self._ik:                                                     # validates ik_options; no device call
            self._ik[key] = IKSolver(self._sys_rrt.robot, [o for o in self._pobs], joint_limits=self._ik_limits, njoint=self.nj,
                                     device=self.device, **ik_options)
        ik = self._ik[key]
        if approach is not None:
            with_meshes = bool(approach_meshes and self._meshes)                    # without meshes: the line-only path
            ckey = ("approach", key, int(approach_steps), with_meshes, tuple(sorted((k, repr(v)) for k, v in approach_options.items())))
            if ckey not in self._ik:                                                # validates approach_options; no device call
                shared = {k: v for k, v in ik_options.items() if k in ("tool", "tool_axis", "tol_pos", "tol_axis", "weight")}
                self._ik[ckey] = CartesianPath(self._sys_rrt.robot, [o for o in self._pobs], joint_limits=self._ik_limits, njoint=self.nj,
                                               device=self.device, steps=int(approach_steps), meshes=with_meshes, **shared, **approach_options)
            cart = self._ik[ckey]
        timer = self._timer(approach_timing, "approach_timing", ik_options, int(approach_steps), int(approach_steps) + 1)
        auditor, asub = self._auditor(approach_audit, "approach_audit", ik_options)
        stream = _args.as_stream(stream, self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            dev = [self._on_device(a, S) for a in args]
            x0, tp, ta = dev[0], dev[1], dev[2] if len(dev) > 2 else None
            if approach is None:                              # `src` supplies ok and goal: the IK launch, or the trace behind it
                src = sol = ik.solve_device(tp, ta, x0, seed=int(seed), stream=stream)
                more = {}
            else:
                u = self._on_device(adir, S)
                u = u / torch.linalg.norm(u, dim=1, keepdim=True)
                dd = dist if isinstance(dist, torch.Tensor) else torch.tensor(dist, dtype=torch.float64, device=self.device)
                pre = (tp - dd.reshape(-1, 1) * u).contiguous()
                sol = ik.solve_device(pre, ta, x0, seed=int(seed), want_candidates=True, stream=stream)
                src = cart.trace_device(sol.cand_theta, tp, ta, x0, start_state=sol.cand_status, want_candidates=auditor is not None, stream=stream)
                ik_ok = sol.status == 0
                if auditor is not None:
                    src, no_pass, audited = self._audit_choice(cart, auditor, asub, sol.cand_theta, src, x0, stream, "approach")
                more = dict(ik_goal=sol.theta, approach_path=src.path, grasp=src.path[:, -1], approach_status=src.status,
                            approach_clearance=src.clearance, approach_selected=src.selected)
                if timer is not None:
                    tm = timer.time_device(src.path, state=src.status, steps=int(approach_steps), stream=stream)
                    more.update(approach_time=tm.time, approach_sdot=tm.sdot, approach_duration=tm.duration, approach_time_status=tm.status)
            ok = src.status == 0
            if approach is not None and auditor is not None:
                ok = ok & ~no_pass
            goal = torch.where(ok[:, None], src.theta, x0)
            res = self.plan(x0, goal, seed, **dict(plan_kwargs, stream=stream))
            masked = torch.full_like(res.status, -2)          # a slot without a goal is masked: -2 no IK solution, -3 no approach
            if approach is not None:
                masked = torch.where(ik_ok, torch.full_like(res.status, -3), masked)
                if auditor is not None:
                    masked = torch.where(no_pass, torch.full_like(res.status, -4), masked)
                    more.update(audited)
            res.status = torch.where(ok, res.status, masked)
            res.has_solution = torch.where(ok, res.has_solution, torch.zeros_like(res.has_solution))
            res.selected = torch.where(ok, res.selected, torch.full_like(res.selected, -1))
            res.goal, res.ik_status, res.ik_err_pos, res.ik_clearance = src.theta, sol.status, sol.err_pos, sol.clearance
            vars(res).update(more)
        return res

    # ---- tool paths ----------------------------------------------------------------------------------------------------------
    def plan_to_path(self, x0, path_pos, path_axis, seed=0, ik_options=None, ik_meshes=False, path_steps=4, path_options=None,
                     path_meshes=False, path_timing=None, path_audit=None, **plan_kwargs):
        """plan() to the start of a tool path that can be followed to its end: path_pos (S, M, 3) or (M, 3), the points the tool
        passes, path_axis the same shape, the tool direction at each (cart.CartesianPath.follow; include/cfs_hip.h, "Tool paths").
        One IK launch at the first pose (path_pos[:, 0], path_axis[:, 0]) with its candidates kept (theta_ref = x0, ik_options as
        for plan_to_pose), one follow_device launch from every candidate (cand_theta / cand_status) along the whole polyline on the
        same stream (path_steps sub-steps per segment; path_options: CartesianPath's max_iter, max_joint_step; tool, tolerances
        and weight are ik_options'; theta_ref = x0), then plan(x0, goal, seed, **plan_kwargs) with row 0 of the winners' paths as
        goals: per slot the IK candidate nearest to x0 from which the whole path exists inside the joint ranges, without a joint
        jump and free of the cell.
        Returns plan()'s namespace plus tool_path (S, N, 5; N = (M-1)*path_steps + 1), tool_path_status (CartesianPath's status),
        tool_path_clearance, tool_path_selected, ik_goal (IK's own winner), ik_status, ik_err_pos, ik_clearance and goal (the
        configuration planned to: tool_path[:, 0]; NaN rows without one).  A slot without an IK solution is planned with goal = x0
        and masked with status = -2, a slot with one but with no candidate that follows the path with status = -3 (has_solution =
        0, selected = -1), exactly as plan_to_pose masks them.
        A planner with mesh obstacles refuses unless ik_meshes=True and path_meshes=True; both solvers are then built from the
        planner's whole cell, as plan_to_pose(..., approach_meshes=True) builds them.  On a planner without meshes they are the
        line-only paths.
        path_timing: None (the default: everything above, bit for bit) or a dict of timing.PathTimer's vmax, amax (both needed),
        feed, stops, curve_share (the tool point is ik_options'): the winners' paths are then timed on the same stream
        (stops="corners": at rest at every pose of the polyline, which needs path_steps >= 2), and the result gains tool_path_time,
        tool_path_sdot (S, N), tool_path_duration and tool_path_time_status (PathTimer's status).  A slot masked -2 / -3 holds NaN
        rows and status 1.  Needs N >= 3.
        path_audit: None (the default: everything above, bit for bit) or a dict of substeps (default 8), min_clearance, max_chord
        (audit.PathAudit's; a missing one is not tested; the tool point is ik_options'): the path is then followed with every
        candidate kept, all of them are audited between their rows on the same stream (include/cfs_hip.h, "Tool-path audit"), and
        per slot the candidate nearest to x0 -- follow's own cost -- among those that pass is taken: tool_path, tool_path_clearance,
        tool_path_selected and goal are that candidate's.  A slot with a complete candidate none of which passes gets status = -4 and
        is masked like -3; its tool_path stays follow's own winner, the path that failed.  The result gains tool_path_clear_lower,
        tool_path_clear_path, tool_path_chord_err, tool_path_chord_upper and tool_path_audit_state (PathAudit's state_out) of the
        path reported.  With both thresholds off every field equals the unaudited call's.  A planner with meshes refuses."""
        if path_audit is not None and self._meshes:
            raise ValueError("path_audit on a planner with mesh obstacles: meshes are not audited between the rows (line obstacles only)")
        for flag, name in ((ik_meshes, "ik_meshes"), (path_meshes, "path_meshes")):
            if not isinstance(flag, bool):
                raise ValueError(f"{name} must be True or False, not {flag!r}")
        if self._meshes and not ik_meshes:
            raise ValueError("plan_to_path on a planner with mesh obstacles needs ik_meshes=True: the default IK collision test reads "
                             "line obstacles only")
        if self._meshes and not path_meshes:
            raise ValueError("plan_to_path on a planner with mesh obstacles needs path_meshes=True: the default path test reads line "
                             "obstacles only")
        _args.int_in(path_steps, "path_steps", 1, MAX_STEPS)
        _args.int_in(seed, "seed", 0)
        if ik_options is None:
            ik_options = {}
        if not isinstance(ik_options, dict) or set(ik_options) - {"tool", "tool_axis", "restarts", "max_iter", "tol_pos", "tol_axis", "weight"}:
            raise ValueError("ik_options must be a dict of IKSolver's tool, tool_axis, restarts, max_iter, tol_pos, tol_axis, weight")
        if path_options is None:
            path_options = {}
        if not isinstance(path_options, dict) or set(path_options) - {"max_iter", "max_joint_step"}:
            raise ValueError("path_options must be a dict of CartesianPath's max_iter, max_joint_step")
        stream = plan_kwargs.get("stream")
        if stream is not None:
            _args.as_stream(stream, self.device)
        x0 = self._conv(x0, "x0", self.nj)
        if path_axis is None:
            raise ValueError("plan_to_path needs path_axis: the tool direction at every pose of the path")
        pp, pa = self._conv(path_pos, "path_pos", 3, table=True), self._conv(path_axis, "path_axis", 3, nonzero=True, table=True)
        if tuple(pp.shape) != tuple(pa.shape):
            raise ValueError(f"path_pos and path_axis disagree: {tuple(pp.shape)} vs {tuple(pa.shape)}")
        M = pp.shape[-2]
        if not 2 <= M <= MAX_STEPS + 1 or (M - 1) * int(path_steps) > MAX_STEPS:
            raise ValueError(f"a path holds 2..{MAX_STEPS + 1} poses and (poses - 1) * path_steps <= {MAX_STEPS}, not {M} poses x {path_steps} steps")
        rows = {a.shape[0] for a, nd in ((x0, 2), (pp, 3)) if a.ndim == nd}
        if len(rows) > 1:
            raise ValueError(f"x0 and path_pos disagree on S: {sorted(rows)}")
        S = rows.pop() if rows else 1
        if S < 1 or S > self.max_slots:
            raise ValueError(f"S={S} outside 1..max_slots={self.max_slots}")
        key = tuple(sorted((k, repr(v)) for k, v in ik_options.items()))
        if key not in self._ik:                                                     # validates ik_options; no device call
            self._ik[key] = IKSolver(self._sys_rrt.robot, [o for o in self._pobs], joint_limits=self._ik_limits, njoint=self.nj,
                                     device=self.device, **ik_options)
        ik = self._ik[key]
        with_meshes = bool(path_meshes and self._meshes)                            # without meshes: the line-only path
        ckey = ("path", key, int(path_steps), with_meshes, tuple(sorted((k, repr(v)) for k, v in path_options.items())))
        if ckey not in self._ik:                                                    # validates path_options; no device call
            shared = {k: v for k, v in ik_options.items() if k in ("tool", "tool_axis", "tol_pos", "tol_axis", "weight")}
            self._ik[ckey] = CartesianPath(self._sys_rrt.robot, [o for o in self._pobs], joint_limits=self._ik_limits, njoint=self.nj,
                                           device=self.device, steps=int(path_steps), meshes=with_meshes, **shared, **path_options)
        cart = self._ik[ckey]
        timer = self._timer(path_timing, "path_timing", ik_options, int(path_steps), (M - 1) * int(path_steps) + 1)
        auditor, asub = self._auditor(path_audit, "path_audit", ik_options)
        stream = _args.as_stream(stream, self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            x0 = self._on_device(x0, S)
            tabs = []
            for t in (pp, pa):
                if not isinstance(t, torch.Tensor):
                    t = torch.tensor(t, dtype=torch.float64, device=self.device)
                tabs.append((t.unsqueeze(0).expand(S, -1, -1) if t.ndim == 2 else t).contiguous())
            pp, pa = tabs
            sol = ik.solve_device(pp[:, 0].contiguous(), pa[:, 0].contiguous(), x0, seed=int(seed), want_candidates=True, stream=stream)
            src = cart.follow_device(sol.cand_theta, pp, pa, x0, start_state=sol.cand_status, want_candidates=auditor is not None, stream=stream)
            if auditor is not None:
                src, no_pass, audited = self._audit_choice(cart, auditor, asub, sol.cand_theta, src, x0, stream, "tool_path")
            ok, ik_ok = src.status == 0, sol.status == 0
            first = src.path[:, 0]
            goal = torch.where(ok[:, None], first, x0)
            res = self.plan(x0, goal, seed, **dict(plan_kwargs, stream=stream))
            masked = torch.where(ik_ok, torch.full_like(res.status, -3), torch.full_like(res.status, -2))
            if auditor is not None:
                masked = torch.where(no_pass, torch.full_like(res.status, -4), masked)
                ok = ok & ~no_pass
            res.status = torch.where(ok, res.status, masked)
            res.has_solution = torch.where(ok, res.has_solution, torch.zeros_like(res.has_solution))
            res.selected = torch.where(ok, res.selected, torch.full_like(res.selected, -1))
            res.goal, res.ik_goal, res.ik_status, res.ik_err_pos, res.ik_clearance = first, sol.theta, sol.status, sol.err_pos, sol.clearance
            res.tool_path, res.tool_path_status, res.tool_path_clearance, res.tool_path_selected = src.path, src.status, src.clearance, src.selected
            if auditor is not None:
                vars(res).update(audited)
            if timer is not None:
                tm = timer.time_device(src.path, state=src.status, steps=int(path_steps), stream=stream)
                res.tool_path_time, res.tool_path_sdot, res.tool_path_duration, res.tool_path_time_status = tm.time, tm.sdot, tm.duration, tm.status
        return res

    def _auditor(self, audit, name, ik_options):
        """(the PathAudit, the sub-steps) of a path_audit / approach_audit dict ((None, None): no audit), validated without a device
        call"""
        if audit is None:
            return None, None
        if not isinstance(audit, dict) or set(audit) - {"substeps", "min_clearance", "max_chord"}:
            raise ValueError(f"{name} must be a dict of substeps, min_clearance, max_chord")
        substeps = _args.int_in(audit.get("substeps", 8), f"{name}['substeps']", 1, MAX_SUBSTEPS)
        key = (name, repr(ik_options.get("tool")), repr(audit.get("min_clearance")), repr(audit.get("max_chord")))
        if key not in self._ik:
            self._ik[key] = PathAudit(self._sys_rrt.robot, [o for o in self._pobs], tool=ik_options.get("tool"), njoint=self.nj, device=self.device,
                                      min_clearance=audit.get("min_clearance"), max_chord=audit.get("max_chord"))
        return self._ik[key], substeps

    def _audit_choice(self, cart, auditor, substeps, starts, src, x0, stream, prefix):
        """Audits every candidate of a trace / follow result `src` (made with want_candidates) and takes, per slot, the passing
        candidate of the smallest cost -- the kernels' own: sum_c w_c (start_c - x0_c)^2 in joint order, the lowest index on a tie.
        Returns (src with theta, path, clearance and selected of that candidate where it is not the kernel's own winner, the slots
        that have a complete candidate but none that passes, the audit's outputs of the path reported as a dict of result fields)."""
        au = auditor.audit_device(src.cand_path, state=src.cand_status, substeps=substeps, stream=stream)
        w = np.ones(self.nj) if cart.weight is None else cart.weight
        cost = torch.zeros_like(au.clear_lower)
        for c in range(self.nj):                              # one rounding per operation, as ik_cost has them
            dl = starts[:, :, c] - x0[:, None, c]
            cost = cost + float(w[c]) * (dl * dl)
        passing = au.state_out == 0
        idx = torch.where(passing, cost, torch.full_like(cost, math.inf)).argmin(dim=1)
        passed = passing.any(dim=1)
        complete = src.status == 0
        take = passed & (idx != src.selected)                 # another candidate than the kernel's winner
        pick = lambda t, i: t.gather(1, i.reshape((-1,) + (1,) * (t.ndim - 1)).expand((-1, 1) + tuple(t.shape[2:]))).squeeze(1)  # noqa: E731
        out = SimpleNamespace(**vars(src))
        out.theta = torch.where(take[:, None], pick(starts, idx), src.theta)
        out.path = torch.where(take[:, None, None], pick(src.cand_path, idx), src.path)
        out.clearance = torch.where(take, pick(au.clear_rows, idx), src.clearance)
        out.selected = torch.where(take, idx.to(src.selected.dtype), src.selected)
        shown = torch.where(passed, idx, src.selected.clamp(min=0).to(idx.dtype))
        audited = {f"{prefix}_{k}": pick(getattr(au, k), shown) for k in ("clear_lower", "clear_path", "chord_err", "chord_upper")}
        audited[f"{prefix}_audit_state"] = pick(au.state_out, shown)
        return out, complete & ~passed, audited

    def _timer(self, timing, name, ik_options, steps, rows):
        """the PathTimer of a path_timing / approach_timing dict (None: no timing), validated without a device call"""
        if timing is None:
            return None
        if not isinstance(timing, dict) or set(timing) - {"vmax", "amax", "feed", "stops", "curve_share"} or not {"vmax", "amax"} <= set(timing):
            raise ValueError(f"{name} must be a dict of PathTimer's vmax and amax, and optionally feed, stops, curve_share")
        if not MIN_ROWS <= rows <= MAX_ROWS:
            raise ValueError(f"{name}: a timed path has {MIN_ROWS}..{MAX_ROWS} rows, not {rows}")
        key = (name, repr(ik_options.get("tool")), tuple(sorted((k, repr(v)) for k, v in timing.items())))
        if key not in self._ik:
            self._ik[key] = PathTimer(self._sys_rrt.robot, njoint=self.nj, device=self.device, tool=ik_options.get("tool"), **timing)
        self._ik[key]._stop_every(steps)                                            # stops="corners" with one sub-step is refused here
        return self._ik[key]

    # ---- the pipeline ----------------------------------------------------------------------------------------------------
    def plan(self, x0, goal, seed, max_rounds=50, stream=None, want_candidates=False, max_draws=None, timings=None):
        """Plan S slots: x0, goal (S, 5) or (5,) (one shared pair), CUDA tensors on the planner's device or array-likes.
        seed: the library's counter-based RRT generator; round r grows its trees with seed + r*ROUND_SEED_STRIDE, tree index
        s*K + k in round 0 and (rank of slot s among the slots still open)*K + k later.  max_draws: uniforms a tree may consume
        (cfs_rrt_desc.max_draws; default the library's).  Returns a namespace of CUDA tensors, one row per slot:
          u, x_, cost_all, e_cost_all, e_u_all, cost (final cost cost_all[iter_O-2], NaN without one), iter_O, total_iter,
          status (-1: no route found), has_solution (1: status 0/1, or 4 when no seed reached 0/1), selected (seed k, -1: no
          route), route (S, MAX_ITER+1, 5) / route_len (the selected route; 0 rows without one), rounds;
          on "soften" also viol_all, n_soft; with min_clearance also dist_path, dist_lower (S, nobs; NaN without a route) and
          clearance_ok (1: the kept candidate keeps margin - slack along its motion).
        want_candidates: also .candidates -- the S*K solve outputs (select="best"), route, route_len, route_ok of every seed.
        timings: a dict to receive the milliseconds of the grow / build / solve / select parts (events on the stream; with
        min_clearance also audit)."""
        _args.int_in(seed, "seed", 0)
        _args.int_in(max_rounds, "max_rounds", 1)
        if max_draws is not None:
            _args.int_in(max_draws, "max_draws", 1)
        if timings is not None and not isinstance(timings, dict):
            raise ValueError("timings must be a dict")
        S, x0, goal = self._pair(x0, goal)
        stream = _args.as_stream(stream, self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            return self._plan(S, self._on_device(x0, S), self._on_device(goal, S), int(seed), int(max_rounds), stream,
                              want_candidates, max_draws, timings)

    def _plan(self, S, x0, goal, seed, max_rounds, stream, want_candidates, max_draws, timings):
        K, N, nj, dev, st = self.K, self.N, self.nj, self.device, stream.cuda_stream
        ev = {}
        mark = (lambda k: ev.setdefault(k, torch.cuda.Event(enable_timing=True)).record(stream)) if timings is not None else (lambda k: None)
        i32 = dict(dtype=torch.int32, device=dev)
        mark("grow0")
        # ---- grow: rounds of K seeds per open slot (s_Parallel_rrt.m:14-28) ----
        SK = S * K
        route = torch.zeros(SK, N, nj, dtype=torch.float64, device=dev)
        route_len = torch.zeros(SK, **i32)
        route_ok = torch.zeros(SK, **i32)
        rounds = torch.zeros(S, **i32)
        open_slots = torch.arange(S, device=dev)
        kk = torch.arange(K, device=dev)
        for r in range(max_rounds):
            n_open = int(open_slots.numel())
            if n_open == 0:
                break
            tx0 = x0[open_slots].repeat_interleave(K, 0).contiguous()
            tg = goal[open_slots].repeat_interleave(K, 0).contiguous()
            g = self.rrt.grow_device(n_open * K, seed + r * ROUND_SEED_STRIDE, dev, max_draws=max_draws, x0=tx0, goal=tg, stream=st)
            ok = (g.fail == 0).view(n_open, K)
            slot_ok = ok.any(dim=1)
            rounds[open_slots] = r + 1
            dst = (open_slots[:, None] * K + kk[None, :])[slot_ok].reshape(-1)     # candidate rows of the slots done this round
            src = (torch.arange(n_open, device=dev)[:, None] * K + kk[None, :])[slot_ok].reshape(-1)
            route[dst] = g.route[src]
            route_len[dst] = g.route_len[src]
            route_ok[dst] = ok.reshape(-1)[src].to(torch.int32)
            open_slots = open_slots[~slot_ok]                                     # boolean index: the one host read of a round
        # failed trees: the 2-point placeholder start -> goal keeps the batch at S*K problems; they are never selected
        bad = route_ok == 0
        route[:, 0] = torch.where(bad[:, None], x0.repeat_interleave(K, 0), route[:, 0])
        route[:, 1] = torch.where(bad[:, None], goal.repeat_interleave(K, 0), route[:, 1])
        route_len = torch.where(bad, torch.full_like(route_len, 2), route_len)
        mark("build0")
        viol = None
        if self.select == "best":
            terms = self.cfs.build_terms_from_ragged_routes_device(route, route_len, stream=st)
            mark("solve0")
            cand = self.cfs.solve_device(*terms, self._obs[:SK], stream=st)
            if self.on_infeasible == "soften":
                v, ns = self.cfs.soft_results(SK)
                viol, n_soft = torch.tensor(v, device=dev), torch.tensor(ns, device=dev)
            rows_ok, kpick = route_ok, None
        else:
            lens = torch.where(route_ok != 0, route_len, torch.full_like(route_len, torch.iinfo(torch.int32).max)).view(S, K)
            kpick = torch.argmin(lens, dim=1)                                         # first minimum: the first seed wins ties
            found = route_ok.view(S, K).any(dim=1)
            pick = torch.arange(S, device=dev) * K + kpick
            terms = self.cfs.build_terms_from_ragged_routes_device(route[pick].contiguous(), route_len[pick].contiguous(), stream=st)
            mark("solve0")
            cand = self.cfs.solve_device(*terms, self._obs[:S], stream=st)
            if self.on_infeasible == "soften":
                v, ns = self.cfs.soft_results(S)
                viol, n_soft = torch.tensor(v, device=dev), torch.tensor(ns, device=dev)
            rows_ok = found.to(torch.int32)                                         # the K = 1 selection gathers the S rows
        Kc = K if self.select == "best" else 1
        aud = None
        if self.min_clearance is not None:                                            # one launch over every solved candidate
            mark("audit0")
            audit = self.cfs.clearance_mesh_device if self._meshes else self.cfs.clearance_device
            aud = audit(cand.x_, cand.u, terms[1], self._obs[:S * Kc], substeps=self.audit_substeps, stream=st)
            clear_ok = (aud.dist_path >= self.cfs._margin_on(dev)[None, :] - self.min_clearance).all(dim=1)
        mark("select0")

        def pick(ok):
            o = self.cfs.alloc_outputs(S, dev)
            o.status.fill_(-1)
            o.selected, o.has_solution = torch.empty(S, **i32), torch.empty(S, **i32)
            o.viol = torch.zeros(S, self.cfs.K, dtype=torch.float64, device=dev) if viol is not None else None
            select_best_device(self.cfs, S, Kc, ok, cand, o, o.selected, o.has_solution, viol, o.viol, stream=st)
            return o
        if aud is None:
            best = pick(rows_ok)
        else:
            # eligible = found and clear; a slot that comes back empty although a seed found a route takes the plain rule's
            # candidate, without a solution (cfs_select_best_device itself is unchanged)
            best, plain = pick(rows_ok * clear_ok.to(torch.int32)), pick(rows_ok)
            fall = (best.selected < 0) & (plain.selected >= 0)
            for name in tuple(SOLVE_OUT) + ("selected",) + (("viol",) if viol is not None else ()):
                a, b2 = getattr(best, name), getattr(plain, name)
                setattr(best, name, torch.where(fall.view(-1, *([1] * (a.ndim - 1))), b2, a))
            best.has_solution = torch.where(fall, torch.zeros_like(best.has_solution), best.has_solution)
        selected, has_solution, best_viol = best.selected, best.has_solution, best.viol
        del best.selected, best.has_solution, best.viol
        mark("end")
        if aud is not None:                                                           # the kept candidate's audit
            krow = torch.arange(S, device=dev) * Kc + selected.clamp(min=0).long()
            kept = (selected >= 0)
            nan = torch.full((S, self.cfs.nobs), float("nan"), dtype=torch.float64, device=dev)
            best.dist_path = torch.where(kept[:, None], aud.dist_path[krow], nan)
            best.dist_lower = torch.where(kept[:, None], aud.dist_lower[krow], nan)
            best.clearance_ok = (kept & clear_ok[krow]).to(torch.int32)
        if kpick is not None:                                                         # shortest: the seed is the argmin
            selected = torch.where(selected >= 0, kpick.to(torch.int32), selected)
        have = selected >= 0
        crow = torch.arange(S, device=dev) * K + selected.clamp(min=0)
        res = best
        it = res.iter_O.long()
        res.cost = torch.where(it >= 2, res.cost_all.gather(1, (it - 2).clamp(min=0)[:, None])[:, 0],
                               torch.full_like(res.cost_all[:, 0], float("nan")))
        res.has_solution, res.selected, res.rounds = has_solution, selected, rounds
        res.route = torch.where(have[:, None, None], route[crow], torch.zeros_like(route[crow]))
        res.route_len = torch.where(have, route_len[crow], torch.zeros_like(route_len[crow]))
        if viol is not None:
            res.viol_all = best_viol
            nrow = crow if self.select == "best" else torch.arange(S, device=dev)
            res.n_soft = torch.where(have, n_soft[nrow], torch.zeros_like(n_soft[nrow]))
        if want_candidates:
            c = SimpleNamespace(route=route, route_len=route_len, route_ok=route_ok)
            if self.select == "best":
                vars(c).update({k: getattr(cand, k) for k in SOLVE_OUT})
                if viol is not None:
                    c.viol_all, c.n_soft = viol, n_soft
                if aud is not None:
                    c.xR1, c.dist_path, c.dist_lower, c.clear_ok = terms[1], aud.dist_path, aud.dist_lower, clear_ok.to(torch.int32)
            res.candidates = c
        if timings is not None:
            stream.synchronize()
            timings.update(grow=ev["grow0"].elapsed_time(ev["build0"]), build=ev["build0"].elapsed_time(ev["solve0"]),
                           solve=ev["solve0"].elapsed_time(ev.get("audit0", ev["select0"])), select=ev["select0"].elapsed_time(ev["end"]))
            if "audit0" in ev:
                timings["audit"] = ev["audit0"].elapsed_time(ev["select0"])
        return res
