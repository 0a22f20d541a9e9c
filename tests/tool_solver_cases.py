"""Cases of tests/test_gpu_tool_solver.py: inverse kinematics, Cartesian lines and tool paths (polylines), line-only and in a mesh cell,
at the shapes that reach every piece the two units share (csrc/cfs_ik_dev.h: the workgroup staging, the convergence test, the cost, the
wave argmin; the iteration around them, which stands in cfs_ik_kernel and in cfs_cart_kernel; csrc/cfs_mesh_hit_dev.h: the mesh decision
with its overflow fallback, the winner's mesh clearance) and both kinds of path of cfs_cart_kernel<NJ, POLY>.
Shared by the test and by tests/tools/record_tool_solver.py, which designs the inputs and writes them and the parent build's outputs
to tests/golden/tool_solver_*.npy; the test reads the inputs back, so it does not depend on how this machine rounds them.

  T = 5 leaves the last workgroup with one of its four wavefronts in use; 7 restarts / candidates leave 57 idle lanes in the argmin.
  M16iB (six joints, axis mode) is the instantiation at the register limit (cfs_cart_kernel<6, *> are the ones with scratch); 2L has
  two joints and no axis.  `states`: candidate states that the recording of the case holds (test_recordings_reach_the_states).
  A mesh case runs under three flag settings: the default, variant A ("per_lane") and variant B with the 8-entry frontier
  ("small_frontier": the overflow fallback decides; tool_solver_overflows.json holds the counter of every recorded run), and once
  more without its mesh ("line"), so that the recordings themselves show which candidates the mesh rejected.
  A "follow" case is a polyline of M poses with K sub-steps per segment ((M-1)K + 1 rows).  K = 2 puts a row on and a row off a table
  pose in every segment; K = 1 makes every row a table pose and advances the segment at every row.  State 4 includes a start farther than
  max_joint_step from its row-0 solution (cand_done 0, no row), state 3 the middle row of two exactly opposite consecutive axes."""
import numpy as np

import rrt_mesh_reference as M

GOLDEN_PREFIX = "tool_solver_"
MESH_VARIANTS = (None, "per_lane", "small_frontier")   # mesh_variant of the solver
LINE = "line"                                           # the mesh case without its mesh
OVERFLOWS = "tool_solver_overflows.json"                # {case: {flag setting: frontier overflows of the recorded run}}
LINE_ONLY = (None,)

# case -> keywords.  kind: "ik" | "cart" | "follow"; R: restarts | candidates; K: steps (follow: per segment of the M poses); mesh: the
# cylinder of rrt_mesh_reference behind the lines; reach (rad), D (m): the spacing of a designed polyline's poses and its obstacle's margin
CASES = {
    "ik_m200i_5x64": dict(kind="ik", robot="M200i", nj=5, axis=True, T=5, R=64, max_iter=12, seed=3, nobs=1, states=(0, 1, 2)),
    "ik_m200i_3x7": dict(kind="ik", robot="M200i", nj=5, axis=True, T=3, R=7, max_iter=100, seed=4, nobs=0, states=(0, 1)),
    "ik_m16ib_5x64": dict(kind="ik", robot="M16iB", nj=6, axis=True, T=5, R=64, max_iter=12, seed=5, nobs=1, states=(0, 1, 2)),
    "ik_m16ib_3x7": dict(kind="ik", robot="M16iB", nj=6, axis=True, T=3, R=7, max_iter=100, seed=6, nobs=0, states=(0,)),
    "ik_2l_5x64": dict(kind="ik", robot="2L", nj=2, axis=False, T=5, R=64, max_iter=12, seed=7, nobs=1, states=(0, 1, 2)),
    "ik_2l_3x7": dict(kind="ik", robot="2L", nj=2, axis=False, T=3, R=7, max_iter=100, seed=8, nobs=0, states=(0,)),
    "ik_mesh_5x64": dict(kind="ik", robot="M200i", nj=5, axis=True, T=5, R=64, max_iter=100, seed=11, nobs=1, mesh=True, states=(0, 2)),
    "cart_m200i_5x64x8": dict(kind="cart", robot="M200i", nj=5, axis=True, T=5, R=64, K=8, max_iter=20, max_joint_step=0.2, nobs=1,
                              states=(0, 1, 2, 4, 5)),
    "cart_m200i_3x7x2": dict(kind="cart", robot="M200i", nj=5, axis=True, T=3, R=7, K=2, max_iter=20, max_joint_step=0.1, nobs=1,
                             states=(0, 1, 2, 4, 5)),
    "cart_m16ib_5x64x8": dict(kind="cart", robot="M16iB", nj=6, axis=True, T=5, R=64, K=8, max_iter=20, max_joint_step=0.2, nobs=1,
                              states=(0, 1, 2, 4, 5)),
    "cart_m16ib_3x7x2": dict(kind="cart", robot="M16iB", nj=6, axis=True, T=3, R=7, K=2, max_iter=20, max_joint_step=0.1, nobs=1,
                             states=(0, 1, 2, 4, 5)),
    "cart_2l_5x64x8": dict(kind="cart", robot="2L", nj=2, axis=False, T=5, R=64, K=8, max_iter=20, max_joint_step=0.2, nobs=1, tol_pos=1e-3,
                           states=(0, 1, 2, 5)),
    "cart_2l_3x7x2": dict(kind="cart", robot="2L", nj=2, axis=False, T=3, R=7, K=2, max_iter=20, max_joint_step=0.05, nobs=1, tol_pos=1e-3,
                          states=(0, 1, 2, 4, 5)),
    "cart_mesh_3x64x8": dict(kind="cart", robot="M200i", nj=5, axis=True, T=3, R=64, K=8, max_iter=20, max_joint_step=0.2, nobs=1, mesh=True,
                             states=(0, 2, 5)),
    "follow_m200i_5x64x3x2": dict(kind="follow", robot="M200i", nj=5, axis=True, T=5, R=64, M=3, K=2, reach=0.25, D=0.01, max_iter=20,
                                  max_joint_step=0.2, nobs=1, states=(0, 1, 2, 3, 4, 5)),
    "follow_m200i_3x7x4x1": dict(kind="follow", robot="M200i", nj=5, axis=True, T=3, R=7, M=4, K=1, reach=0.25, D=0.01, max_iter=20,
                                 max_joint_step=0.4, nobs=1, states=(0, 1, 2, 4, 5)),
    "follow_m16ib_5x64x3x2": dict(kind="follow", robot="M16iB", nj=6, axis=True, T=5, R=64, M=3, K=2, reach=0.25, D=0.01, max_iter=20,
                                  max_joint_step=0.2, nobs=1, states=(0, 1, 2, 3, 4, 5)),
    "follow_2l_5x64x3x2": dict(kind="follow", robot="2L", nj=2, axis=False, T=5, R=64, M=3, K=2, reach=0.1, D=0.004, max_iter=20,
                               max_joint_step=0.2, nobs=1, tol_pos=1e-3, states=(0, 1, 2, 4, 5)),
    "follow_mesh_3x64x3x4": dict(kind="follow", robot="M200i", nj=5, axis=True, T=3, R=64, M=3, K=4, max_iter=20, max_joint_step=0.2, nobs=1,
                                 mesh=True, states=(0, 2, 5)),
}
RUNS = [(c, v) for c, kw in CASES.items() for v in ((LINE,) + MESH_VARIANTS if kw.get("mesh") else LINE_ONLY)]
IK_OUT = ("theta", "status", "selected", "n_ok", "err_pos", "err_axis", "clearance", "cand_theta", "cand_status", "cand_iter")
CART_OUT = ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance", "cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")


def out_fields(case):
    return IK_OUT if CASES[case]["kind"] == "ik" else CART_OUT


def rows(case):
    """rows of a path of the case"""
    c = CASES[case]
    return (c["M"] - 1) * c["K"] + 1 if c["kind"] == "follow" else c["K"] + 1


def in_dtype(case):
    """one record per target; the line obstacles of the case are repeated in every record"""
    c = CASES[case]
    nj, R, nobs = c["nj"], c["R"], c["nobs"]
    if c["kind"] == "follow":
        d = [("path_pos", "<f8", (c["M"], 3)), ("path_axis", "<f8", (c["M"], 3))]
    else:
        d = [("target_pos", "<f8", (3,)), ("target_axis", "<f8", (3,))]
    d += [("theta_ref", "<f8", (nj,)), ("obs", "<f8", (nobs, 6)), ("D", "<f8", (nobs,))]
    if c["kind"] != "ik":
        d += [("start", "<f8", (R, nj)), ("start_state", "<i4", (R,))]
    return d


def out_dtype(case):
    c = CASES[case]
    nj, R = c["nj"], c["R"]
    if c["kind"] == "ik":
        return [("theta", "<f8", (nj,)), ("status", "<i4"), ("selected", "<i4"), ("n_ok", "<i4"), ("err_pos", "<f8"), ("err_axis", "<f8"),
                ("clearance", "<f8"), ("cand_theta", "<f8", (R, nj)), ("cand_status", "<i4", (R,)), ("cand_iter", "<i4", (R,))]
    K1 = rows(case)
    return [("theta", "<f8", (nj,)), ("status", "<i4"), ("path", "<f8", (K1, nj)), ("selected", "<i4"), ("n_ok", "<i4"), ("n_done", "<i4"),
            ("clearance", "<f8"), ("cand_status", "<i4", (R,)), ("cand_done", "<i4", (R,)), ("cand_iter", "<i4", (R,)),
            ("cand_end", "<f8", (R, nj)), ("cand_path", "<f8", (R, K1, nj))]


def golden_name(case, variant=None, inputs=False):
    return f"{GOLDEN_PREFIX}{case}_in.npy" if inputs else f"{GOLDEN_PREFIX}{case}_{variant or 'default'}_out.npy"


def obstacles(pkg, case, rec, with_mesh=True):
    """the obs cell of the case: the recorded lines, then (mesh cases, unless with_mesh is false) the cylinder"""
    c = CASES[case]
    obs = [dict(l=np.stack([rec["obs"][0, j, :3], rec["obs"][0, j, 3:]], axis=1), D=float(rec["D"][0, j])) for j in range(c["nobs"])]
    if c.get("mesh") and with_mesh:
        obs.append(dict(mesh=pkg.Mesh(tri=M.scene_triangles()), D=M.CYL_D))
    return obs


def run(pkg, case, variant, rec):
    """the case's solver on the recorded inputs through the host-array entry, every optional output requested: one record per target"""
    c = CASES[case]
    mesh = bool(c.get("mesh")) and variant != LINE
    variant = None if variant == LINE else variant
    robot, obs = pkg.robotproperty2(c["robot"]), obstacles(pkg, case, rec, mesh)
    pos, axis = ("path_pos", "path_axis") if c["kind"] == "follow" else ("target_pos", "target_axis")
    tp, tr = np.ascontiguousarray(rec[pos]), np.ascontiguousarray(rec["theta_ref"])
    ta = np.ascontiguousarray(rec[axis]) if c["axis"] else None
    tol = dict(tol_pos=c.get("tol_pos", 1e-6), tol_axis=1e-6)
    if c["kind"] == "ik":
        slv = pkg.IKSolver(robot, obs or None, restarts=c["R"], max_iter=c["max_iter"], njoint=c["nj"], mesh_variant=variant, **tol)
        r = slv.solve(tp, ta, tr, seed=c["seed"], want_candidates=True)
    else:
        slv = pkg.CartesianPath(robot, obs or None, steps=c["K"], max_iter=c["max_iter"], max_joint_step=c["max_joint_step"], njoint=c["nj"],
                                meshes=mesh, mesh_variant=variant, **tol)
        call = slv.follow if c["kind"] == "follow" else slv.trace
        r = call(np.ascontiguousarray(rec["start"]), tp, ta, tr, start_state=np.ascontiguousarray(rec["start_state"]), want_candidates=True)
    out = np.zeros(rec.shape[0], dtype=out_dtype(case))
    for k in out_fields(case):
        out[k] = getattr(r, k)
    return out


def overflows(pkg, case, reset=False):
    """the frontier-overflow counter of the case's unit (cfs_debug_ik_frontier_overflows | cfs_debug_cart_frontier_overflows)"""
    import ctypes as C
    from motionplanning_5d_m_amd import _lib
    n = C.c_ulonglong(0)
    unit = "ik" if CASES[case]["kind"] == "ik" else "cart"
    _lib.check(getattr(_lib.lib(), f"cfs_debug_{unit}_frontier_overflows")(C.byref(n), 1 if reset else 0))
    return int(n.value)
