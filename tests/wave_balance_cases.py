"""Problem families of tests/test_gpu_wave_balance.py: shapes at which the placement of the fused solver's riding work (the QP's
start vector and its two rollouts, `prep(1..3)` of csrc/cfs_fused.hip, on the wavefronts that the linearisation phase they ride on
leaves with a pass less) takes another path.  Shared by the test and by tests/tools/record_wave_balance.py,
which designs the problems and writes inputs and the parent build's outputs to tests/golden/wave_balance_*.npy; the test reads the
inputs back, so it does not depend on how this machine rounds them.

First wavefront that carries the riding work (0: all four, the mapping from before), from the item counts of tile 0 -- chain
`Wc * (2 nj + 1)` (analytic: `Wc`), base distances `nj * Wc * nobs`, minima `Wc * nobs`, `Wc` the tile's waypoints:

  case        nj  H  nobs  rows  tile 0   chain / base / minima items   prep(1) / prep(2) / prep(3) start on wavefront
  5x30x8       5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (config 3's shape; on w1: old mapping)
  5x30x8still  5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (start = goal: the skipped-step branch)
  2x12x1       2  12   1    96     12         60 /   24 /  12             1 / 1 / 1     (two joints on six half-waves)
  5x31x7       5  31   7   160     16        176 /  560 / 112             3 / 1 / 2     (tile 1 has 15 waypoints: not consulted)
  6x40x3       6  40   3   256     14        any                          0 / 0 / 0     (H > 32: one joint per wavefront, unchanged)
  5x30x8a      5  30   8   160     15         15 /  600 / 120             1 / 2 / 2     (analytic Jacobian)
  5x30x8m      5  30   8   160   narrower    by the plan                  by the counts (per-waypoint obstacles: more tiles)
  5x30x8l      5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (joint position limits)

(tests/test_wave_balance_rule.py restates the rule and checks these rows.)  Only the kernels of the identity Hessian's half-CU tier
(w2s: every `PSGCFS default` run below) are compiled with the new placement (`CFS_RIDE_IDLE`).  The `CFS default` runs (w2m) and the
`w1` runs execute the mapping from before whatever the table says for their shape: w2m was measured slower with the new placement,
w1 was not timed; they are recorded here so that they stay pinned if that changes.  Noise variants of a PSGCFS run: "full" (12 rows, one per
possible iteration), "short" (3 rows: iterations 4.. take the `have == false` branch of prep(2)), "none"."""
import numpy as np

B = 6
MARGIN = 0.1
M200I_X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])
NOISE_ROWS = {"full": 12, "short": 3}

# case -> (robot, nj, H, nobs, CFSBatch keywords, [(mode, tier, noise variant)])
PLAIN = [("PSGCFS", "default", "full"), ("CFS", "default", "none")]
CASES = {
    "5x30x8": ("M200i", 5, 30, 8, {}, PLAIN + [("PSGCFS", "default", "short"), ("PSGCFS", "w1", "full"), ("CFS", "w1", "none")]),
    "5x30x8still": ("M200i", 5, 30, 8, {}, [("PSGCFS", "default", "none"), ("PSGCFS", "default", "short")]),
    "2x12x1": ("2L", 2, 12, 1, {}, PLAIN),
    "5x31x7": ("M200i", 5, 31, 7, {}, PLAIN),
    "6x40x3": ("M200i", 6, 40, 3, {}, PLAIN),
    "5x30x8a": ("M200i", 5, 30, 8, dict(jacobian="analytic"), PLAIN),
    "5x30x8m": ("M200i", 5, 30, 8, dict(obstacles="per_waypoint"), PLAIN),
    "5x30x8l": ("M200i", 5, 30, 8, dict(joint_limits="robot"), PLAIN),
}
RUNS = [(c, m, t, z) for c, v in CASES.items() for m, t, z in v[5]]
IN_FIELDS = ("x_init", "xR1", "ff", "caug", "obs")
OUT_FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
MAX_O_ITER = 12


def family(pkg, case):
    """sys_info of the case (weights of tests/lin_decode_cases.py), start and goal"""
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
    _, nj, H, _, _, _ = CASES[case]
    K = MAX_O_ITER
    return [("u", "<f8", (H * nj,)), ("x_", "<f8", (2 * H * nj,)), ("cost_all", "<f8", (K,)), ("e_cost_all", "<f8", (K,)),
            ("e_u_all", "<f8", (K,)), ("iter_O", "<i4"), ("total_iter", "<i4"), ("status", "<i4")]


def noise_of(rec, variant):
    return None if variant == "none" else np.ascontiguousarray(rec["noise"][:, :NOISE_ROWS[variant]])


def run(pkg, case, mode, tier, variant, rec):
    """the case's handle on the recorded inputs: whole solves, one record per problem"""
    s, _, _ = family(pkg, case)
    nobs, kw = CASES[case][3], CASES[case][4]
    n = rec.shape[0]
    h = pkg.CFSBatch(s, nobs, np.full(nobs, MARGIN), mode=mode, max_batch=n, **kw)
    h.debug_options(tier_w1=tier == "w1")
    arg = {k: np.ascontiguousarray(rec[k]) for k in IN_FIELDS}
    r = h.solve(arg["x_init"], arg["xR1"], arg["ff"], arg["caug"], arg["obs"], noise=noise_of(rec, variant) if mode == "PSGCFS" else None)
    out = np.zeros(n, dtype=out_dtype(case))
    for k in OUT_FIELDS:
        out[k] = getattr(r, k)
    h.close()
    return out


def first_free_wavefront(items, threads=256, wave=64):
    """the placement rule restated: threads stride over `items`; the first wavefront with a pass less than wavefront 0, 0 if none"""
    passes = [max(0, -(-(items - wave * w) // threads)) for w in range(threads // wave)]
    return next((w for w in range(1, len(passes)) if passes[w] < passes[0]), 0)


def ride_plan(nj, H, nobs, tile, analytic=False):
    """(prep(1), prep(2), prep(3)) -> first wavefront, as launch_fused_tier packs them for the half-CU tiers"""
    if H > 32:
        return (0, 0, 0)
    chain = tile if analytic else tile * (2 * nj + 1)
    return (first_free_wavefront(chain), first_free_wavefront(nj * tile * nobs), first_free_wavefront(tile * nobs))
