"""The argument, packing and stream plumbing every binding module shares: the Python half of DESIGN.md section 22.

Conversions to what the C ABI reads, the scalar checks with their ValueError, the lookups over the tables of ``_lib``, the device,
stream and tensor rules of the ``_device`` entries, and the split of an obs cell.  Only what two or more entry points use lives
here, and nothing here calls the library: the entry points do, through ``_lib.lib()`` at call time (tests replace it).
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib  # noqa: F401  (imports torch first, see _lib)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


# ---- conversions -------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def ptr(a):
    if a is None:
        return None
    if torch is not None and isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def fill(struct, ns):
    """set every pointer field of the ctypes struct that the namespace has to the address of that array or tensor"""
    have = vars(ns)
    for k, t in struct._fields_:
        if k in have and t is C.c_void_p:
            setattr(struct, k, ptr(have[k]))
    return struct


def zeros_on(device):
    """zeros(shape, numpy dtype): numpy arrays for device None, else torch tensors on that device"""
    if device is None:
        return np.zeros
    return lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=device)


# ---- scalars -----------------------------------------------------------------------------------------------------------------
def is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def int_in(v, name, lo, hi=None):
    """v as an int when it is an integer (not a bool) in lo..hi (hi None: no upper end), else ValueError"""
    if not is_int(v) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer {f'>= {lo}' if hi is None else f'in {lo}..{hi}'}, not {v!r}")
    return int(v)


def real(v, name, positive=True):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{name} must be a finite real number{' > 0' if positive else ''}, not {v!r}")
    return float(v)


# ---- names and codes of the _lib tables --------------------------------------------------------------------------------------
def one_of(names, v, name):
    if not isinstance(v, str) or v not in names:
        raise ValueError(f"{name} must be one of {sorted(names)}, not {v!r}")
    return v


def code(table, v, name):
    return table[one_of(table, v, name)]


def name_of(table, c):
    return {v: k for k, v in table.items()}[c]


# ---- devices, streams, tensors -----------------------------------------------------------------------------------------------
def cuda_device(device):
    """int | str | torch.device -> a CUDA (HIP) torch.device with an index"""
    device = torch.device("cuda", int(device)) if is_int(device) else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"device must be a CUDA (HIP) device, not {device}")
    return torch.device("cuda", 0) if device.index is None else device


def as_stream(stream, device):
    """a torch.cuda.Stream, or None for the current stream of `device`; ValueError for anything else"""
    if stream is None:
        return torch.cuda.current_stream(device)
    if not isinstance(stream, torch.cuda.Stream):
        raise ValueError("stream must be a torch.cuda.Stream")
    return stream


def stream_ptr(stream, device):
    """a raw stream pointer, or None for the pointer of the current stream of `device`"""
    return torch.cuda.current_stream(device).cuda_stream if stream is None else stream


def cuda_tensor(t, name, shape, dtype=None, device=None):
    """t, contiguous, when it is a CUDA tensor of `dtype` (default float64) whose shape matches `shape` (None: any length) and which
    lives on `device` (None: any), else ValueError"""
    dtype = torch.float64 if dtype is None else dtype
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} CUDA tensor")
    if t.ndim != len(shape) or any(w is not None and v != w for v, w in zip(t.shape, shape)):
        raise ValueError(f"{name} must have shape {tuple('T' if w is None else w for w in shape)}, not {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the solver on {device}")
    return t.contiguous()


# ---- obs cells ---------------------------------------------------------------------------------------------------------------
def obs_meshes(obs, poses=False):
    """The Mesh objects of an obs cell; mesh obstacles must come after the line obstacles (cfs_problem_set_meshes).  A mesh entry
    with a pose (a moving mesh, cfs_problem_set_mesh_motion) is refused unless poses=True: only the trajectory solvers have a time
    axis to place it on, and everything else would silently measure the mesh as stored."""
    flags = ["mesh" in o for o in obs]
    if any(flags) and flags != sorted(flags):
        raise ValueError("mesh obstacles must follow the line-segment obstacles in the obs cell")
    if not poses and any("mesh" in o and "pose" in o for o in obs):
        raise ValueError("a mesh obstacle with a pose moves along a trajectory's waypoints: only CFS_FANUC and PSGCFS_FANUC take one "
                         "(RRT, IK, Cartesian paths and the RRT-CFS planner have no time axis; pass the mesh without pose)")
    return [o["mesh"] for o in obs if "mesh" in o]


def split_obs(obs):
    """obs cell -> (line rows (n, 6) [l(:,1); l(:,2)], their D (n,), the Mesh objects, their D (nmesh,)); ValueError when a mesh
    precedes a line obstacle.  Nothing else is checked here: what a D may be is the caller's rule."""
    meshes = obs_meshes(obs)
    lines = [o for o in obs if "mesh" not in o]
    ends = [np.asarray(o["l"], float) for o in lines]
    rows = np.array([np.concatenate([l[:, 0], l[:, 1]]) for l in ends]).reshape(-1, 6)
    return f64(rows), f64([o["D"] for o in lines]), meshes, f64([o["D"] for o in obs if "mesh" in o])


def mesh_table(meshes, D_mesh=None, flags=0):
    """(nmesh, handle array, D_mesh pointer, flags): the mesh table of cfs_problem_set_meshes, cfs_rrt_grow_mesh* and
    cfs_ik_solve_mesh*"""
    arr = (C.c_void_p * max(len(meshes), 1))(*[m._h for m in meshes])
    return len(meshes), arr, ptr(D_mesh), int(flags)
