"""Tool-path audit: what a joint path does between its rows, over ``cfs_path_audit`` (include/cfs_hip.h, "Tool-path audit"; DESIGN.md
section 29).

``CartesianPath.trace`` / ``follow`` and the planner's ``plan_to_pose(approach=)`` / ``plan_to_path`` test their rows against the
obstacles; a controller moves the joints linearly between the rows.  ``PathAudit`` measures that motion on G x R paths of N rows at
once: per path the clearance from the line obstacles and the deviation of the tool point from the chord, each sampled at ``substeps``
points per segment and each with a bound that holds between the samples.  ``cand_path`` with ``cand_status`` of a ``follow`` /
``trace`` call go in as they are, and ``state_out`` goes into ``PathTimer.time(state=)`` as it is.  One wavefront per path; this
module packs arguments and unpacks results, the sampling and the reductions are a HIP kernel (csrc/cfs_audit.hip).
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

MAX_PATHS = 64
MIN_ROWS, MAX_ROWS = 2, 257
MAX_SUBSTEPS = 64


def _threshold(v, name, off, positive):
    """None -> off (no test); else a finite real (positive: > 0)"""
    return off if v is None else _args.real(v, name, positive=positive)


class PathAudit:
    """Audit of joint paths for one robot and one set of line obstacles.

    robot: robotproperty2(id); njoint: joints of the chain, as for IKSolver.  obs: None or the obs cell of line obstacles
    (dict(l=3x2, D=...)) that IKSolver takes; mesh obstacles are not audited and an entry with `mesh` or `pose` is refused.  tool: the
    tool point in the frame of link njoint (default: default_tool).  min_clearance: None (no test) or a finite number of metres: a path
    whose certified clearance is below it gets state_out 6.  max_chord: None (no test) or metres > 0: a path whose certified chord
    deviation is above it gets state_out 7.  Arguments are validated here, before anything touches the device."""

    def __init__(self, robot, obs, tool=None, min_clearance=None, max_chord=None, device=None, njoint=None):
        self.robot, self.nj = robot, _njoint(robot, njoint)
        self.tool = default_tool(robot, self.nj)[0] if tool is None else _vec3(tool, "tool")
        self.min_clearance = _threshold(min_clearance, "min_clearance", -math.inf, False)
        self.max_chord = _threshold(max_chord, "max_chord", math.inf, True)
        try:
            obs = [] if obs is None else list(obs)
        except TypeError:
            raise ValueError(f"obs must be None or a list of line obstacles, not {obs!r}") from None
        if len(obs) > _lib.CFS_MAX_OBS:
            raise ValueError(f"{len(obs)} obstacles: at most {_lib.CFS_MAX_OBS}")
        for j, o in enumerate(obs):
            if not isinstance(o, dict) or "l" not in o and "mesh" not in o:
                raise ValueError(f"obs[{j}] must be a dict(l=3x2, D=...)")
            if "mesh" in o or "pose" in o:
                raise ValueError(f"obs[{j}] is a mesh obstacle: meshes are not audited between the rows (line obstacles only)")
            if np.shape(o["l"]) != (3, 2) or not np.isfinite(np.asarray(o["l"], float)).all():
                raise ValueError(f"obs[{j}]['l'] must be a finite 3x2 array")
            _args.real(o.get("D"), f"obs[{j}]['D']", positive=False)
        self.obs, self.D, _, _ = _args.split_obs(obs)
        if device is not None:
            if torch is None:
                raise ValueError("device= needs torch")
            device = _args.cuda_device(device)
        self.device = device
        self._dev = None                                      # (device, obstacle rows, D) uploaded by the device entry

    def _desc(self, substeps, obs, D):
        d = _lib.cfs_audit_desc()
        d.robot, d.njoint = to_c_robot(self.robot), self.nj
        for q in range(3):
            d.tool[q] = float(self.tool[q])
        d.nobs = int(self.obs.shape[0])
        d.obs, d.D = (_ptr(obs), _ptr(D)) if d.nobs else (None, None)
        d.substeps = _args.int_in(substeps, "substeps", 1, MAX_SUBSTEPS)
        d.min_clearance, d.max_chord = self.min_clearance, self.max_chord
        return d

    def _dims(self, shape):
        """(G, R, N) and the leading shape of the results for paths of `shape`: (N, nj), (T, N, nj) or (T, R, N, nj)"""
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
    def _shapes(G, R):
        f, i = np.float64, np.int32
        return dict(clear_rows=((G, R), f), clear_path=((G, R), f), s_path=((G, R), f), clear_lower=((G, R), f), chord_err=((G, R), f),
                    chord_upper=((G, R), f), link_path=((G, R), i), obs_path=((G, R), i), status=((G, R), i), state_out=((G, R), i))

    @staticmethod
    def _shaped(r, lead):
        for k in vars(r):
            setattr(r, k, getattr(r, k).reshape(lead))
        return r

    # ---- host arrays in and out (cfs_path_audit) ---------------------------------------------------------------------------------
    def audit(self, paths, state=None, substeps=8):
        """Audit paths (N, njoint), (T, N, njoint) or (T, R, N, njoint) -- CartesianPath's path and cand_path --, N in 2..257, R in
        1..64.  state: integers of the leading shape or None: cand_status, a path is audited only when its entry is 0.  substeps:
        1..64 samples per segment.  Returns a namespace of numpy arrays of the leading shape: clear_rows, clear_path, clear_lower
        (metres: the least clearance at the rows, at the samples, and a bound for all of the motion that certifies when it is > 0),
        s_path, link_path, obs_path (where clear_path lies: row number plus fraction, link 1-based, obstacle 0-based), chord_err,
        chord_upper (metres: the largest sampled distance of the tool point from the same-fraction point of the chord, and a bound
        for all of the motion), status (0 audited | 1 not audited | 2 a non-finite row) and state_out (state, then 3 non-finite |
        6 clear_lower < min_clearance | 7 chord_upper > max_chord | 0).  A path that was not audited holds NaN and -1."""
        try:
            p = np.array(paths, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"paths must be an array of shape (N, {self.nj}), (T, N, {self.nj}) or (T, R, N, {self.nj})") from None
        G, R, N, lead = self._dims(p.shape)
        d = self._desc(substeps, self.obs, self.D)
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
        r = SimpleNamespace(**{k: np.zeros(*sd) for k, sd in self._shapes(G, R).items()})
        o = _args.fill(_lib.cfs_audit_out(), r)
        _lib.check(_lib.lib().cfs_path_audit(C.byref(d), G, R, N, _ptr(p), _ptr(ss), C.byref(o)))
        return self._shaped(r, lead)

    # ---- CUDA tensors in and out (cfs_path_audit_device) -------------------------------------------------------------------------
    def audit_device(self, paths, state=None, substeps=8, stream=None):
        """audit() on CUDA tensors of the audit's device: paths float64, state int32 of the leading shape or None; enqueued on
        `stream` (a torch.cuda.Stream; default: the current one) without a host synchronisation."""
        if torch is None:
            raise ValueError("audit_device needs torch")
        if not isinstance(paths, torch.Tensor) or not paths.is_cuda:
            raise ValueError("paths must be a float64 CUDA tensor")
        G, R, N, lead = self._dims(tuple(paths.shape))
        _args.int_in(substeps, "substeps", 1, MAX_SUBSTEPS)
        dev = paths.device
        if self.device is not None and dev != self.device:
            raise ValueError(f"paths is on {dev}, the audit on {self.device}")
        stream = _args.as_stream(stream, dev)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            # checked in here: making a strided input contiguous is a copy, which belongs on the stream that reads it
            p = _args.cuda_tensor(paths, "paths", tuple(paths.shape), device=dev)
            ss = None if state is None else _args.cuda_tensor(state, "state", lead, torch.int32, device=dev)
            if self._dev is None or self._dev[0] != dev:      # the obstacles are uploaded once per device
                self._dev = (dev, torch.tensor(self.obs, dtype=torch.float64, device=dev), torch.tensor(self.D, dtype=torch.float64, device=dev))
            d = self._desc(substeps, self._dev[1], self._dev[2])
            z = _args.zeros_on(dev)
            r = SimpleNamespace(**{k: z(*sd) for k, sd in self._shapes(G, R).items()})
            o = _args.fill(_lib.cfs_audit_out(), r)
            _lib.check(_lib.lib().cfs_path_audit_device(C.byref(d), G, R, N, _ptr(p), _ptr(ss), C.byref(o), C.c_void_p(stream.cuda_stream)))
            for t in (p, ss, paths, state) + self._dev[1:]:
                if t is not None:
                    t.record_stream(stream)
        return self._shaped(r, lead)
