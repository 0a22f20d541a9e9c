"""Developer aid (GPU): writes the recordings tests/test_gpu_tool_solver.py compares against -- tests/golden/tool_solver_*.npy -- with
whatever library is given (default libcfs_hip.so; a file next to it).  They are recorded with a library built from the commit BEFORE
cfs_ik.hip and cfs_cart.hip took their staging, selection and mesh decision from one place:
`make -C motionplanning_5d_m_amd/csrc OUTNAME=libcfs_hip_parent.so` at that commit.  The follow_* cases were added later and are
recorded, by the same recipe, with a library built from the commit BEFORE the line and the polyline kernel became one
(cfs_cart_kernel<NJ, POLY>): `only=follow_` writes them alone and leaves every other recording as it is.
usage: python tests/tools/record_tool_solver.py [libname.so] [outdir] [only=CASE_PREFIX]

`<case>_in.npy` holds the inputs, one record per target (designed here from the scene builders of tests/ik_reference.py,
tests/ik_mesh_reference.py and tests/cart_mesh_reference.py); `<case>_<flags>_out.npy` the outputs of
tests/tool_solver_cases.run; `tool_solver_overflows.json` the frontier-overflow counter after every run of a mesh case.  The printout shows the
candidate states of every recording."""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

from motionplanning_5d_m_amd import _lib
LIBNAME = next((a for a in sys.argv[1:] if a.endswith(".so")), "libcfs_hip.so")
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), LIBNAME)          # before the first lib() call
GOLDEN = os.path.join(os.path.dirname(HERE), "golden")
ONLY = next((a[5:] for a in sys.argv[1:] if a.startswith("only=")), "")
OUT = next((a for a in sys.argv[1:] if not a.endswith(".so") and not a.startswith("only=")), GOLDEN)
import motionplanning_5d_m_amd as pkg
from oracle import oracle as O
import cart_mesh_reference as CM
import ik_mesh_reference as K
import ik_reference as R
import tool_solver_cases as W

O.build()


def _through(point, D, half=0.5):
    """a vertical line obstacle of 2 * half m through `point` (tests/test_gpu_ik.py::test_infeasible_targets's): rows (1, 6), (1,)"""
    return np.concatenate([point - np.array([0, 0, half]), point + np.array([0, 0, half])])[None], np.array([D])


def design_ik(case):
    c = W.CASES[case]
    rec = np.zeros(c["T"], dtype=W.in_dtype(case))
    if c.get("mesh"):                                            # the scene of tests/test_gpu_ik_mesh.py, its first T targets
        arm, lim, lines, tri, inp = K.scene()
        rec["target_pos"], rec["target_axis"], rec["theta_ref"] = inp.target_pos[:c["T"]], inp.target_axis[:c["T"]], inp.theta_ref[:c["T"]]
        rec["obs"], rec["D"] = K.obs_rows(lines)
        return rec
    lim = np.asarray(pkg.robotproperty2(c["robot"]).thetamax, float)[:c["nj"]]
    arm = R.Arm(O.robotproperty2(c["robot"]), c["nj"])
    salt = zlib.crc32(case.encode()) % 1000
    q = R.in_limit_configs(lim, c["T"], salt)
    poses = [arm.pose(x) for x in q]
    rec["target_pos"], rec["target_axis"] = np.array([p for p, _ in poses]), np.array([a for _, a in poses])
    rec["theta_ref"] = R.in_limit_configs(lim, c["T"], salt + 1, shrink=0.6)
    if c["nobs"]:                                                # through target 0's tool point: its converged restarts collide
        rec["obs"], rec["D"] = _through(rec["target_pos"][0], 0.1)
    return rec


def _mesh_scene(rec, T, Rn):
    """the scene of tests/test_gpu_cart_mesh.py into rec: the starts are the candidates of the line-only inverse kinematics at the
    pre-grasp poses; returns (the scene's inputs, the cylinder's triangles)"""
    arm, lim, lines, tri, inp = CM.scene()
    ik = pkg.IKSolver(pkg.robotproperty2("M200i"), lines, restarts=Rn, max_iter=inp.ik_max_iter, tol_pos=inp.tol_pos, tol_axis=inp.tol_axis)
    sol = ik.solve(inp.pre_pos[:T], inp.pre_axis[:T], inp.theta_ref[:T], seed=CM.SEED, want_candidates=True)
    rec["start"], rec["start_state"], rec["theta_ref"] = sol.cand_theta, sol.cand_status, inp.theta_ref[:T]
    rec["obs"], rec["D"] = K.obs_rows(lines)
    return inp, tri


def design_cart(case):
    c = W.CASES[case]
    T, Rn, nj = c["T"], c["R"], c["nj"]
    rec = np.zeros(T, dtype=W.in_dtype(case))
    if c.get("mesh"):
        inp, _ = _mesh_scene(rec, T, Rn)
        rec["target_pos"], rec["target_axis"] = inp.target_pos[:T], inp.target_axis[:T]
        return rec
    # tests/test_gpu_cart.py::_case's recipe: targets are poses of configurations near the first candidate of their row; the other
    # candidates are configurations near that one and, every fifth, a random one far away
    lim = np.asarray(pkg.robotproperty2(c["robot"]).thetamax, float)[:nj]
    arm = R.Arm(O.robotproperty2(c["robot"]), nj)
    salt = zlib.crc32(case.encode()) % 1000
    rng = np.random.default_rng(salt)
    q = R.in_limit_configs(lim, T, salt, shrink=0.6)
    start = q[:, None, :] + 0.03 * rng.standard_normal((T, Rn, nj))
    start[:, 0] = q
    far = R.in_limit_configs(lim, T * Rn, salt + 1, shrink=0.9).reshape(T, Rn, nj)
    start[:, 4::5] = far[:, 4::5]
    start = np.clip(start, lim[:, 0], lim[:, 1])
    goal = np.clip(q + 0.15 * (2 * rng.random((T, nj)) - 1), lim[:, 0], lim[:, 1])
    poses = [arm.pose(x) for x in goal]
    tp, ta = np.array([p for p, _ in poses]), np.array([a for _, a in poses])
    state = np.zeros((T, Rn), np.int32)
    start[0, 1, 0] = lim[0, 1] + 0.5                             # a row out of range: no start (state 5)
    state[:, 2] = 1                                              # a candidate inverse kinematics did not solve: no start (state 5)
    tp[T - 1] += np.array([10.0, 0.0, 0.0])                      # out of reach: the first step does not converge (state 1)
    p0, _ = arm.pose(q[1])                                       # on target 1's own line, half way (tests/test_gpu_cart.py::
    rec["obs"], rec["D"] = _through(0.5 * (p0 + tp[1]), 0.04)    # test_collision_on_the_line's): state 2
    rec["start"], rec["start_state"], rec["target_pos"], rec["target_axis"] = start, state, tp, ta
    rec["theta_ref"] = R.in_limit_configs(lim, T, salt + 2, shrink=0.6)
    return rec


def design_follow(case):
    c = W.CASES[case]
    T, Rn, nj, Mp, Ks = c["T"], c["R"], c["nj"], c["M"], c["K"]
    rec = np.zeros(T, dtype=W.in_dtype(case))
    if c.get("mesh"):                                            # tests/test_gpu_cart_follow.py's L past the cylinder: design_cart's starts,
        inp, tri = _mesh_scene(rec, T, Rn)                      # the scene's own approach, then 0.2 m towards the cylinder's axis, which
        to = np.asarray(tri, float).reshape(-1, 3).mean(axis=0)[None, :] - inp.target_pos[:T]   # ends every candidate; the last target
        to[:, 2] = 0.0                                                                          # (the approach nothing touches) backs
        to /= np.linalg.norm(to, axis=1, keepdims=True)                                         # 0.05 m away instead and keeps its winner
        to *= np.where(np.arange(T) == T - 1, -0.05, 0.2)[:, None]
        rec["path_pos"] = np.stack([inp.pre_pos[:T], inp.target_pos[:T], inp.target_pos[:T] + to], axis=1)
        rec["path_axis"] = np.stack([inp.pre_axis[:T]] * 3, axis=1)
        return rec
    # tests/test_gpu_cart_follow.py::_case's recipe: pose 0 is the pose of candidate 0, pose j the pose of a configuration `reach` rad
    # (per joint, at most) from the one before it; the other candidates lie near candidate 0 (they do not solve pose 0 and iterate to
    # it inside the jump bound) and, every fifth, far away (farther than max_joint_step from their row-0 solution: state 4, no row)
    lim = np.asarray(pkg.robotproperty2(c["robot"]).thetamax, float)[:nj]
    arm = R.Arm(O.robotproperty2(c["robot"]), nj)
    salt = zlib.crc32(case.encode()) % 1000
    rng = np.random.default_rng(salt)
    q = R.in_limit_configs(lim, T, salt, shrink=0.6)
    start = q[:, None, :] + 0.03 * rng.standard_normal((T, Rn, nj))
    start[:, 0] = q
    far = R.in_limit_configs(lim, T * Rn, salt + 1, shrink=0.9).reshape(T, Rn, nj)
    start[:, 4::5] = far[:, 4::5]
    start = np.clip(start, lim[:, 0], lim[:, 1])
    way = np.zeros((T, Mp, nj))
    way[:, 0] = q
    for j in range(1, Mp):
        way[:, j] = np.clip(way[:, j - 1] + c["reach"] * (2 * rng.random((T, nj)) - 1), lim[:, 0], lim[:, 1])
    poses = [arm.pose(x) for x in way.reshape(-1, nj)]
    pp, pa = np.array([p for p, _ in poses]).reshape(T, Mp, 3), np.array([a for _, a in poses]).reshape(T, Mp, 3)
    state = np.zeros((T, Rn), np.int32)
    start[0, 1, 0] = lim[0, 1] + 0.5                             # a row out of range: no start (state 5)
    state[:, 2] = 1                                              # a candidate inverse kinematics did not solve: no start (state 5)
    pp[T - 1, Mp - 1] += np.array([10.0, 0.0, 0.0])              # the last pose out of reach: a row of the last segment does not converge (state 1)
    # 10 cm through the first row of target 1's last segment (K = 2: between two table poses), its margin below the rows' spacing:
    # state 2 past a segment boundary (on the 2L, whose rows lie millimetres apart, at the boundary)
    rec["obs"], rec["D"] = _through(pp[1, Mp - 2] + (pp[1, Mp - 1] - pp[1, Mp - 2]) / Ks, c["D"], half=0.05)
    if c["axis"] and Ks == 2:                                    # exactly opposite axes on target 2's last two poses: the middle row of
        pa[2, Mp - 1] = -pa[2, Mp - 2]                           # that segment has |b| = 0 exactly (state 3, follow_row's false return)
    rec["start"], rec["start_state"], rec["path_pos"], rec["path_axis"] = start, state, pp, pa
    rec["theta_ref"] = R.in_limit_configs(lim, T, salt + 2, shrink=0.6)
    return rec


DESIGN = dict(ik=design_ik, cart=design_cart, follow=design_follow)

if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    counts = {}
    if ONLY and os.path.exists(os.path.join(GOLDEN, W.OVERFLOWS)):                # the counters of the recordings that stay
        with open(os.path.join(GOLDEN, W.OVERFLOWS)) as f:
            counts = json.load(f)
    for case, c in W.CASES.items():
        if not case.startswith(ONLY):
            continue
        rec = DESIGN[c["kind"]](case)
        np.save(os.path.join(OUT, W.golden_name(case, inputs=True)), rec)
        for variant in ((W.LINE,) + W.MESH_VARIANTS if c.get("mesh") else W.LINE_ONLY):
            if c.get("mesh"):
                W.overflows(pkg, case, reset=True)
            out = W.run(pkg, case, variant, rec)
            np.save(os.path.join(OUT, W.golden_name(case, variant)), out)
            states = {int(s): int((out["cand_status"] == s).sum()) for s in np.unique(out["cand_status"])}
            note = ""
            if c.get("mesh"):
                counts.setdefault(case, {})[variant or "default"] = W.overflows(pkg, case)
                note = f", frontier overflows {counts[case][variant or 'default']}"
            print(f"{case} {variant or 'default'} ({LIBNAME}): status {out['status'].tolist()}, selected {out['selected'].tolist()}, "
                  f"candidate states {states}{note}", flush=True)
            missing = [] if variant == W.LINE else [s for s in c["states"] if s not in states]
            if missing:
                print(f"  !! states {missing} claimed in tests/tool_solver_cases.py do not occur", flush=True)
    with open(os.path.join(OUT, W.OVERFLOWS), "w") as f:
        json.dump(counts, f, indent=1)
        f.write("\n")
