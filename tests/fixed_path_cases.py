"""Problem families of tests/test_gpu_fixed_path.py: the smallest shapes at which the part of the fused solver that every outer
iteration pays whatever its QP does -- the kinematic chains of the linearisation and the post phase (new u, rollout, get_cost) with
the start vector of the next QP, csrc/cfs_fused.hip; DESIGN.md section 4.1 -- takes another path.  Shared by the test and by
tests/tools/record_fixed_path.py, which designs the problems and writes inputs and the parent build's outputs to
tests/golden/fixed_path_*.npy; the test reads the inputs back, so it does not depend on how this machine rounds them.

  case         nj  H  nobs  rows  what it reaches
  5x30x8        5  30   8   160   config 3's shape: PSGCFS on the half-CU tier with a noise row per iteration, with 3 rows (`have ==
                                  false` in prep(2)) and without noise; CFS (the `x0` branch, `ff` from global memory); both on w1
  5x30x8still   5  30   8   160   start = goal far from every obstacle: the skipped-step branch (x_ is the rollout of the unchanged u)
  2x12x1        2  12   1    96   the two-link arm: the other `kind` (`t2l` link transforms, which stay on fk_step), a chain of 2 joints
  3x30x2        3  30   2    96   the first 3 joints of the M200i: one tile for the whole horizon
  5x31x7        5  31   7   160   tiles of 16 + 15: the last tile's Wc != W
  6x40x3        6  40   3   256   H > 32: one joint per wavefront in the cost scans, register P columns, `ff` from global memory
  5x30x8a       5  30   8   160   analytic Jacobian: the `arm_chain` site
  5x30x8m       5  30   8   160   per-waypoint obstacles (MOVE kernels)
  5x30x8l       5  30   8   160   joint position limits (LIM kernels)
  5x30x8d       5  30   8   160   PSGCFS with `use_weights=False`: the dense QQ product, the other cost branch that reads `ff`

Cases in LIN also record the linearisation of x_init (`cfs_linearize`: dist, grad, link ids), so that a chain error is localised.
Noise variants of a PSGCFS run: "full" (12 rows, one per possible iteration), "short" (3 rows), "none"."""
import numpy as np

B = 6
MARGIN = 0.1
M200I_X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])
NOISE_ROWS = {"full": 12, "short": 3}
MAX_O_ITER = 12

# case -> (robot, nj, H, nobs, CFSBatch keywords, [(mode, tier, noise variant)])
PLAIN = [("PSGCFS", "default", "full"), ("CFS", "default", "none")]
CASES = {
    "5x30x8": ("M200i", 5, 30, 8, {}, PLAIN + [("PSGCFS", "default", "short"), ("PSGCFS", "default", "none"),
                                                ("PSGCFS", "w1", "full"), ("CFS", "w1", "none")]),
    "5x30x8still": ("M200i", 5, 30, 8, {}, [("PSGCFS", "default", "none")]),
    "2x12x1": ("2L", 2, 12, 1, {}, PLAIN),
    "3x30x2": ("M200i", 3, 30, 2, {}, PLAIN),
    "5x31x7": ("M200i", 5, 31, 7, {}, PLAIN),
    "6x40x3": ("M200i", 6, 40, 3, {}, PLAIN),
    "5x30x8a": ("M200i", 5, 30, 8, dict(jacobian="analytic"), PLAIN),
    "5x30x8m": ("M200i", 5, 30, 8, dict(obstacles="per_waypoint"), PLAIN),
    "5x30x8l": ("M200i", 5, 30, 8, dict(joint_limits="robot"), PLAIN),
    "5x30x8d": ("M200i", 5, 30, 8, dict(use_weights=False), [("PSGCFS", "default", "full")]),
}
LIN = ("2x12x1", "5x31x7", "6x40x3")
RUNS = [(c, m, t, z) for c, v in CASES.items() for m, t, z in v[5]]
LIN_RUNS = [r for r in RUNS if r[0] in LIN]
IN_FIELDS = ("x_init", "xR1", "ff", "caug", "obs")
OUT_FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
LIN_FIELDS = ("dist", "grad", "linkid")


def family(pkg, case):
    """sys_info of the case (weights of tests/wave_balance_cases.py), start and goal"""
    rid, nj, H = CASES[case][:3]
    robot = pkg.robotproperty2(rid)
    if rid == "2L":
        x0, xg = np.zeros(2), np.array([np.pi / 2, 0.0])
        kw = dict(Qp=np.diag([10.0, 1.0]), Qv=np.diag([10.0, 1.0]), Rblk=np.diag([5.0, 4.0]), cR=0.1, lim=np.ones(2),
                  max_input_blk=np.ones(2) * 0.25, epsilon_O=1e-6, MAX_O_ITER=MAX_O_ITER)
    else:
        x0 = M200I_X0[:nj]
        xg = x0 * np.array([-1.0, 1, 1, 1, 1, 1])[:nj]
        if case.endswith("still"):
            xg = x0.copy()
        kw = dict(Qp=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Qv=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Rblk=np.eye(nj) * 2, cR=50.0,
                  lim=np.ones(nj), max_input_blk=np.ones(nj), epsilon_O=0.1, MAX_O_ITER=MAX_O_ITER)
    return pkg.build_sys_info(robot, nj, H, x0, xg, pkg.line_reference(x0, xg, H), **kw), x0, xg


def in_dtype(case):
    _, nj, H, nobs, kw, _ = CASES[case]
    oshape = (H, nobs, 6) if kw.get("obstacles") == "per_waypoint" else (nobs, 6)
    return [("x_init", "<f8", (2 * H * nj,)), ("xR1", "<f8", (2 * nj,)), ("ff", "<f8", (H * nj,)), ("caug", "<f8"), ("obs", "<f8", oshape),
            ("noise", "<f8", (NOISE_ROWS["full"], H * nj))]


def out_dtype(case):
    _, nj, H, nobs, _, _ = CASES[case]
    K = MAX_O_ITER
    lin = [("dist", "<f8", (nobs, H)), ("grad", "<f8", (nobs, H, nj)), ("linkid", "<i4", (nobs, H))] if case in LIN else []
    return [("u", "<f8", (H * nj,)), ("x_", "<f8", (2 * H * nj,)), ("cost_all", "<f8", (K,)), ("e_cost_all", "<f8", (K,)),
            ("e_u_all", "<f8", (K,)), ("iter_O", "<i4"), ("total_iter", "<i4"), ("status", "<i4")] + lin


def noise_of(rec, variant):
    return None if variant == "none" else np.ascontiguousarray(rec["noise"][:, :NOISE_ROWS[variant]])


def run(pkg, case, mode, tier, variant, rec):
    """the case's handle on the recorded inputs: whole solves (LIN cases: and the linearisation of x_init), one record per problem"""
    s, _, _ = family(pkg, case)
    nobs, kw = CASES[case][3], CASES[case][4]
    n = rec.shape[0]
    h = pkg.CFSBatch(s, nobs, np.full(nobs, MARGIN), mode=mode, max_batch=n, **kw)
    h.debug_options(tier_w1=tier == "w1")
    arg = {k: np.ascontiguousarray(rec[k]) for k in IN_FIELDS}
    out = np.zeros(n, dtype=out_dtype(case))
    if case in LIN:
        out["dist"], out["linkid"], out["grad"] = h.linearize(arg["x_init"], arg["obs"])
    r = h.solve(arg["x_init"], arg["xR1"], arg["ff"], arg["caug"], arg["obs"], noise=noise_of(rec, variant) if mode == "PSGCFS" else None)
    for k in OUT_FIELDS:
        out[k] = getattr(r, k)
    h.close()
    return out
