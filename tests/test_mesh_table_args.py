"""cfs_rrt_grow_mesh(_device) and cfs_ik_solve_mesh(_device) check their mesh tables with one function: one list of malformed tables,
driven through both families, is refused with CFS_ERR_INVALID_ARG and the same message (up to the lower bound of nmesh, 0 for RRT and
1 for IK) before anything is written.  Host-only refusals come before the comparison of a mesh's device.  No compute calls here (CPU)."""
import ctypes as C
import math

import numpy as np

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import _lib
from test_ik_args import _desc as _ik_desc
from test_rrt_mesh_args import _FakeMesh, _desc as _rrt_desc

M0, M5 = _FakeMesh(), _FakeMesh(device=5)
MANY = _lib.CFS_MAX_OBS                                                  # both descriptors hold one line obstacle: 1 + 32 > CFS_MAX_OBS

# (nmesh, meshes, D_mesh, flags, what the message must name)
MALFORMED = [
    (2, [M0, M0], [0.1, 0.2], 8, b"unknown flags"),                     # unknown flag bits
    (2, [M0, M0], [0.1, 0.2], 16, b"unknown flags"),
    (2, [M0, M0], [0.1, 0.2], -1, b"unknown flags"),
    (2, [M0, M0], [0.1, 0.2], 1 | 2, b"excludes"),                      # both variants
    (2, [M0, M0], [0.1, 0.2], 1 | 4, b"excludes"),                      # variant A with B's small frontier
    (2, None, [0.1, 0.2], 0, b"must be given"),                         # a NULL table
    (2, [M0, M0], None, 0, b"must be given"),
    (2, [M0, None], [0.1, 0.2], 0, b"mesh 1 is NULL"),                  # a NULL entry
    (2, [M0, M0], [0.1, 0.0], 0, b"D_mesh[1]"),
    (2, [M0, M0], [0.1, -0.1], 0, b"D_mesh[1]"),
    (2, [M0, M0], [0.1, math.nan], 0, b"D_mesh[1]"),
    (2, [M0, M0], [0.1, math.inf], 0, b"D_mesh[1]"),
    (MANY, [M0] * MANY, [0.1] * MANY, 0, b"nmesh"),                      # nobs + nmesh > CFS_MAX_OBS
    (-1, [M0], [0.1], 0, b"nmesh"),
    (2, [M5, M0], [0.1, math.nan], 0, b"D_mesh[1]"),                    # two errors: the host-only one is named, not mesh 0's device
    (2, [M5, M0], [0.1, 0.2], 0, b"mesh 0 lives on device 5"),          # ... which is compared last
]


def _table(meshes, D):
    arr = None if meshes is None else (C.c_void_p * max(len(meshes), 1))(*[None if m is None else m._h for m in meshes])
    Dm = None if D is None else np.ascontiguousarray(D, float)
    return arr, Dm, (None if Dm is None else Dm.ctypes.data_as(C.c_void_p))


class _Rrt:
    lower = b"outside 0.."

    def __init__(self):
        self.d, self.o, self.keep = _rrt_desc()
        self.z = self.keep[1]                                            # the one buffer behind every output array
        self.z[:] = 7.0

    def call(self, nmesh, meshes, D, flags, dev):
        lib = pkg.lib()
        arr, Dm, Dp = _table(meshes, D)
        if dev:
            rc = lib.cfs_rrt_grow_mesh_device(C.byref(self.d), nmesh, arr, Dp, flags, 1, C.byref(self.o), None)
        else:
            rc = lib.cfs_rrt_grow_mesh(C.byref(self.d), nmesh, arr, Dp, flags, 1, C.byref(self.o))
        return rc, lib.cfs_last_error()

    def untouched(self):
        return bool((self.z == 7.0).all())


class _Ik:
    lower = b"outside 1.."

    def __init__(self):
        self.slv, self.d, self.o, self.z, self.zi = _ik_desc()
        self.tp, self.tr = np.ones((2, 3)), np.zeros((2, 5))
        self.z[:] = 7.0
        self.zi[:] = 7

    def call(self, nmesh, meshes, D, flags, dev):
        lib = pkg.lib()
        arr, Dm, Dp = _table(meshes, D)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        if dev:
            rc = lib.cfs_ik_solve_mesh_device(C.byref(self.d), nmesh, arr, Dp, flags, 2, p(self.tp), p(self.tp), p(self.tr), C.byref(self.o), None)
        else:
            rc = lib.cfs_ik_solve_mesh(C.byref(self.d), nmesh, arr, Dp, flags, 2, p(self.tp), p(self.tp), p(self.tr), C.byref(self.o))
        return rc, lib.cfs_last_error()

    def untouched(self):
        return bool((self.z == 7.0).all() and (self.zi == 7).all())


def test_both_families_refuse_the_same_tables_with_the_same_message_and_write_nothing():
    rrt, ik = _Rrt(), _Ik()
    assert rrt.d.nobs == ik.d.nobs == 1
    for nmesh, meshes, D, flags, names in MALFORMED:
        for dev in (False, True):
            got = []
            for fam in (rrt, ik):
                rc, err = fam.call(nmesh, meshes, D, flags, dev)
                assert rc == -1 and names in err, (fam.__class__.__name__, dev, nmesh, flags, rc, err)
                assert fam.untouched()
                got.append(err.replace(fam.lower, b"outside N.."))
            assert got[0] == got[1], got
    # the two-error case names D_mesh, never the device of mesh 0
    for fam in (rrt, ik):
        for dev in (False, True):
            rc, err = fam.call(2, [M5, M0], [0.1, -1.0], 0, dev)
            assert rc == -1 and b"D_mesh[1]" in err and b"device" not in err


def test_no_meshes_is_a_table_for_rrt_and_not_for_ik():
    """nothing may be launched here: RRT's call goes on to its next refusal, the incomplete output, which comes after the mesh table"""
    rrt, ik = _Rrt(), _Ik()
    rrt.o.route = None
    for dev in (False, True):
        rc, err = ik.call(0, None, None, 0, dev)
        assert rc == -1 and b"nmesh 0 outside 1.." in err and ik.untouched()
        rc, err = rrt.call(0, None, None, 0, dev)
        assert rc == -1 and b"NULL output array" in err and rrt.untouched()      # the table was accepted
        rc, err = rrt.call(0, None, None, 8, dev)
        assert rc == -1 and b"unknown flags" in err                             # ... and is still read when it is empty
