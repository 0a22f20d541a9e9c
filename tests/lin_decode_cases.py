"""Problem families of tests/test_gpu_lin_decode.py: shapes at which the decode of the fused solver's linearisation work items
(csrc/cfs_fused.hip: item e -> obstacle, waypoint of the tile, link) can go wrong.  Shared by the test and
by tests/tools/record_lin_decode.py, which designs the obstacles with the CPU oracle and writes inputs and outputs to
tests/golden/lin_decode_*.npy; the test reads the inputs back, so it does not depend on how this machine rounds them.

Tile widths (`lin_w`, from the plan of launch_fused_tier; the half-CU tiers w2s / w2m agree, w1 always has one tile here):

  case      nj  H  nobs  kernel rows  tiles in the default tier     handle
  5x31x7     5  31   7      160        16 + 15 (last shorter)        plain; also run on w1 (one tile of 31) and with pruning off
  2x12x1     2  12   1       96        12 (one tile, one obstacle)   plain (two-link arm)
  6x40x3     6  40   3      256        14 + 14 + 12 (last shorter)   plain; CFS also on w1 (one tile of 40)
  3x20x5     3  20   5       96        20 (one tile)                 plain
  5x31x7m    5  31   7      160        11 + 11 + 9 (last shorter)    per-waypoint obstacles (`m` kernels)
  5x31x7a    5  31   7      160        16 + 15                       analytic Jacobian (`a` kernels)
  5x31x7l    5  31   7      160        16 + 15                       joint position limits (`l` kernels)

(5 x 31 x 7 has two static tiles, not three: 17 waypoints fit a tile, and ceil(31 / 2) = 16.  The static handle with three tiles whose
last one is shorter -- `rc_tile` and `rc_last` differ, and a third tile starts behind two full ones -- is 6x40x3; 5x31x7m is the
same for the per-waypoint kernels.)  Seven obstacles are no power of two
and no divisor of the 256 threads, so an item's (obstacle, waypoint, link) changes in every round of every loop."""
import numpy as np

B = 8
MARGIN = 0.1
M200I_X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])

# case -> (robot, nj, H, nobs, CFSBatch keywords, [(mode, tier)])
BOTH = [("CFS", "default"), ("PSGCFS", "default")]
CASES = {
    "5x31x7": ("M200i", 5, 31, 7, {}, BOTH + [("CFS", "w1"), ("PSGCFS", "w1")]),
    "2x12x1": ("2L", 2, 12, 1, {}, BOTH),
    "6x40x3": ("M200i", 6, 40, 3, {}, BOTH + [("CFS", "w1")]),
    "3x20x5": ("M200i", 3, 20, 5, {}, BOTH),
    "5x31x7m": ("M200i", 5, 31, 7, dict(obstacles="per_waypoint"), BOTH),
    "5x31x7a": ("M200i", 5, 31, 7, dict(jacobian="analytic"), BOTH),
    "5x31x7l": ("M200i", 5, 31, 7, dict(joint_limits="robot"), BOTH),
}
RUNS = [(c, m, t) for c, v in CASES.items() for m, t in v[5]]
IN_FIELDS = ("x_init", "xR1", "ff", "caug", "obs", "noise")


def family(pkg, case):
    """sys_info of the case (weights of tests/test_gpu_tiers.py's single problems)"""
    rid, nj, H = CASES[case][:3]
    robot = pkg.robotproperty2(rid)
    if rid == "2L":
        x0, xg = np.zeros(2), np.array([np.pi / 2, 0.0])
        kw = dict(Qp=np.diag([10.0, 1.0]), Qv=np.diag([10.0, 1.0]), Rblk=np.diag([5.0, 4.0]), cR=0.1, lim=np.ones(2),
                  max_input_blk=np.ones(2) * 0.25, epsilon_O=1e-6, MAX_O_ITER=12)
    else:
        x0 = M200I_X0[:nj]
        xg = x0 * np.array([-1.0, 1, 1, 1, 1, 1])[:nj]
        kw = dict(Qp=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Qv=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Rblk=np.eye(nj) * 2, cR=50.0,
                  lim=np.ones(nj), max_input_blk=np.ones(nj), epsilon_O=0.1, MAX_O_ITER=12)
    return pkg.build_sys_info(robot, nj, H, x0, xg, pkg.line_reference(x0, xg, H), **kw), x0, xg


def in_dtype(case):
    _, nj, H, nobs, kw, _ = CASES[case]
    oshape = (H, nobs, 6) if kw.get("obstacles") == "per_waypoint" else (nobs, 6)
    return [("x_init", "<f8", (2 * H * nj,)), ("xR1", "<f8", (2 * nj,)), ("ff", "<f8", (H * nj,)), ("caug", "<f8"), ("obs", "<f8", oshape),
            ("noise", "<f8", (12, H * nj)), ("two_candidates", "<i4"), ("surrogate", "<i4"), ("idle_links", "<i4")]


def out_dtype(case):
    _, nj, H, nobs, _, _ = CASES[case]
    return [("dist", "<f8", (nobs, H)), ("grad", "<f8", (nobs, H, nj)), ("linkid", "<i4", (nobs, H)), ("u", "<f8", (H * nj,)),
            ("x_", "<f8", (2 * H * nj,)), ("status", "<i4"), ("iter_O", "<i4"), ("total_iter", "<i4")]


def run(pkg, case, mode, tier, rec, no_prune=False, solve=True):
    """the case's handle on the recorded inputs: linearisation of x_init and, if asked, the whole solve, as one record per problem"""
    s, _, _ = family(pkg, case)
    nobs, kw = CASES[case][3], CASES[case][4]
    n = rec.shape[0]
    h = pkg.CFSBatch(s, nobs, np.full(nobs, MARGIN), mode=mode, max_batch=n, **kw)
    h.debug_options(tier_w1=tier == "w1", no_prune=no_prune)
    arg = {k: np.ascontiguousarray(rec[k]) for k in IN_FIELDS}
    out = np.zeros(n, dtype=out_dtype(case))
    out["dist"], out["linkid"], out["grad"] = h.linearize(arg["x_init"], arg["obs"])
    if solve:
        r = h.solve(arg["x_init"], arg["xR1"], arg["ff"], arg["caug"], arg["obs"], noise=arg["noise"] if mode == "PSGCFS" else None)
        for k in ("u", "x_", "status", "iter_O", "total_iter"):
            out[k] = getattr(r, k)
    h.close()
    return out
