"""Path timing: a clock on joint paths over ``cfs_path_time`` (include/cfs_hip.h, "Path timing").

``IKSolver``, ``CartesianPath.trace`` / ``follow`` and the planner's ``plan_to_pose(approach=)`` / ``plan_to_path`` return joint rows
without a clock.  ``PathTimer`` times G x R such paths of N rows at once: per path the fastest pass through its rows that keeps
every joint under its speed (``vmax``, rad/s) and acceleration (``amax``, rad/s^2) limits and the tool point under a feed rate
(``feed``, m/s), at rest at both ends and at the stop rows; per group the path that completes soonest.  ``cand_path`` with
``cand_status`` of a ``follow`` / ``trace`` call go in as they are.  One lane per path; this module packs arguments and unpacks
results, the two passes and the selection are HIP kernels (csrc/cfs_time.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import _args, _lib
from ._args import f64 as _f64, ptr as _ptr
from .ik import _njoint, _vec3, default_tool
from .robotproperty2 import to_c_robot

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_PATHS = 64               # paths per group: one wavefront lane each in the selection
MIN_ROWS, MAX_ROWS = 3, 257


def _limits(v, name, nj):
    try:
        a = np.array(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or {nj} numbers, not {v!r}") from None
    if a.ndim == 0:
        a = np.full(nj, float(a))
    if a.shape != (nj,) or not np.isfinite(a).all() or not (a > 0).all():
        raise ValueError(f"{name} must be a finite number > 0 or {nj} of them, not {v!r}")
    return _f64(a)


class PathTimer:
    """Timing of joint paths for one robot and one set of limits.

    robot: robotproperty2(id); njoint: joints of the chain, as for IKSolver.  vmax (rad/s) / amax (rad/s^2): a number or njoint
    numbers, finite and > 0.  feed: None (no cap) or the largest speed of the tool point in m/s, > 0; tool: the tool point in the
    frame of link njoint (default: default_tool), read with a feed.  curve_share: in (0, 1), the share of amax that following the
    curve may use; the rest changes the speed along it.  stops: "ends" (at rest at the first and the last row only), "corners" (also at
    every row that is a multiple of the `steps` given to time(): the poses of a polyline followed with that many sub-steps), or an
    integer k >= 2 (also at every row that is a multiple of k).  Arguments are validated here, before anything touches the device."""

    def __init__(self, robot, vmax, amax, feed=None, tool=None, curve_share=0.5, stops="ends", device=None, njoint=None):
        self.robot, self.nj = robot, _njoint(robot, njoint)
        self.vmax, self.amax = _limits(vmax, "vmax", self.nj), _limits(amax, "amax", self.nj)
        self.feed = math.inf if feed is None else _args.real(feed, "feed")
        self.tool = default_tool(robot, self.nj)[0] if tool is None else _vec3(tool, "tool")
        self.curve_share = _args.real(curve_share, "curve_share")
        if not self.curve_share < 1.0:
            raise ValueError(f"curve_share must lie in (0, 1), not {curve_share!r}")
        if not (stops in ("ends", "corners") if isinstance(stops, str) else _args.is_int(stops) and stops >= 2):
            raise ValueError(f'stops must be "ends", "corners" or an integer >= 2, not {stops!r}')
        self.stops = stops if isinstance(stops, str) else int(stops)
        if device is not None:
            if torch is None:
                raise ValueError("device= needs torch")
            device = _args.cuda_device(device)
        self.device = device

    def _stop_every(self, steps):
        if steps is not None:
            _args.int_in(steps, "steps", 1)
        if self.stops == "corners":
            if steps is None or steps < 2:
                raise ValueError(f'stops="corners" needs steps >= 2 (the sub-steps per segment of the polyline), not {steps!r}')
            return int(steps)
        return 0 if self.stops == "ends" else self.stops

    def _desc(self, steps):
        d = _lib.cfs_time_desc()
        d.robot, d.njoint = to_c_robot(self.robot), self.nj
        for q in range(3):
            d.tool[q] = float(self.tool[q])
        d.vmax, d.amax = _ptr(self.vmax), _ptr(self.amax)
        d.feed, d.curve_share, d.stop_every = self.feed, self.curve_share, self._stop_every(steps)
        return d

    def _dims(self, shape):
        """(G, R, N) and the leading shape of the per-path results for paths of `shape`: (N, nj), (T, N, nj) or (T, R, N, nj)"""
        nj = self.nj
        if len(shape) not in (2, 3, 4) or shape[-1] != nj:
            raise ValueError(f"paths must have shape (N, {nj}), (T, N, {nj}) or (T, R, N, {nj}), not {tuple(shape)}")
        lead = tuple(shape[:-2])
        G = lead[0] if lead else 1
        R = lead[1] if len(lead) == 2 else 1
        N = shape[-2]
        if G < 1 or not 1 <= R <= MAX_PATHS or not MIN_ROWS <= N <= MAX_ROWS:
            raise ValueError(f"paths {tuple(shape)}: T >= 1, R in 1..{MAX_PATHS} and N in {MIN_ROWS}..{MAX_ROWS} are needed")
        return int(G), int(R), int(N), lead

    @staticmethod
    def _shapes(G, R, N):
        f, i = np.float64, np.int32
        return dict(time=((G, R, N), f), sdot=((G, R, N), f), duration=((G, R), f), status=((G, R), i), selected=((G,), i),
                    group_status=((G,), i))

    @staticmethod
    def _shaped(r, lead, N):
        """the namespace with the caller's leading dimensions: time, sdot lead + (N,); duration, status lead; selected, group_status
        (T,), or () for a single path"""
        grp = lead[:1]
        for k, s in (("time", lead + (N,)), ("sdot", lead + (N,)), ("duration", lead), ("status", lead), ("selected", grp), ("group_status", grp)):
            setattr(r, k, getattr(r, k).reshape(s))
        return r

    # ---- host arrays in and out (cfs_path_time) ----------------------------------------------------------------------------------
    def time(self, paths, state=None, steps=None):
        """Time paths (N, njoint), (T, N, njoint) or (T, R, N, njoint) -- CartesianPath's path and cand_path --, N in 3..257, R in
        1..64.  state: integers of the leading shape or None: cand_status, a path is timed only when its entry is 0.  steps: the
        sub-steps per segment, for stops="corners".  Returns a namespace of numpy arrays: time and sdot (leading shape + (N,): the
        time stamp of every row in seconds and ds/dt there, one unit of s per row), duration and status (leading shape; 0 timed | 1
        not timed | 2 numeric | 3 stalled: two consecutive rows at rest | 4 a repeated row), selected and group_status ((T,), or ()
        for one path: per group the timed path of the smallest duration, -1 / 1 without one).  Rows of a path that was not timed
        hold NaN."""
        try:
            p = np.array(paths, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"paths must be an array of shape (N, {self.nj}), (T, N, {self.nj}) or (T, R, N, {self.nj})") from None
        G, R, N, lead = self._dims(p.shape)
        d = self._desc(steps)
        ss = None
        if state is not None:
            try:
                ss = np.array(state)
            except (TypeError, ValueError):
                raise ValueError("state must be an integer array") from None
            if ss.dtype.kind not in "iu" or ss.shape != lead:
                raise ValueError(f"state must be an integer array of shape {lead}, not {ss.dtype} {ss.shape}")
            ss = np.ascontiguousarray(ss.astype(np.int32))
        p = _f64(p)
        r = SimpleNamespace(**{k: np.zeros(*sd) for k, sd in self._shapes(G, R, N).items()})
        o = _args.fill(_lib.cfs_time_out(), r)
        _lib.check(_lib.lib().cfs_path_time(C.byref(d), G, R, N, _ptr(p), _ptr(ss), C.byref(o)))
        return self._shaped(r, lead, N)

    # ---- CUDA tensors in and out (cfs_path_time_device) --------------------------------------------------------------------------
    def time_device(self, paths, state=None, steps=None, stream=None):
        """time() on CUDA tensors of the timer's device: paths float64, state int32 of the leading shape or None; enqueued on
        `stream` (a torch.cuda.Stream; default: the current one) without a host synchronisation."""
        if torch is None:
            raise ValueError("time_device needs torch")
        if not isinstance(paths, torch.Tensor) or not paths.is_cuda:
            raise ValueError("paths must be a float64 CUDA tensor")
        G, R, N, lead = self._dims(tuple(paths.shape))
        d = self._desc(steps)
        dev = paths.device
        if self.device is not None and dev != self.device:
            raise ValueError(f"paths is on {dev}, the timer on {self.device}")
        stream = _args.as_stream(stream, dev)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            # checked in here: making a strided input contiguous is a copy, which belongs on the stream that reads it
            p = _args.cuda_tensor(paths, "paths", tuple(paths.shape), device=dev)
            ss = None if state is None else _args.cuda_tensor(state, "state", lead, torch.int32, device=dev)
            z = _args.zeros_on(dev)
            r = SimpleNamespace(**{k: z(*sd) for k, sd in self._shapes(G, R, N).items()})
            o = _args.fill(_lib.cfs_time_out(), r)
            _lib.check(_lib.lib().cfs_path_time_device(C.byref(d), G, R, N, _ptr(p), _ptr(ss), C.byref(o), C.c_void_p(stream.cuda_stream)))
            for t in (p, ss, paths, state):
                if t is not None:
                    t.record_stream(stream)
        return self._shaped(r, lead, N)
