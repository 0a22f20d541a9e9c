"""The recorded bit-identity nets of the fused solver (csrc/cfs_fused.hip), in one place.  A change to the
solver that moves no floating-point statement must return, bit for bit, what the kernels returned before it: a suite is a set of
problems designed to reach the paths the change touches, recorded (inputs and outputs, tests/golden/<suite>_*.npy) by
`tests/tools/record_fused.py <suite>` with a library built from the commit BEFORE the change.  tests/test_gpu_fused_recorded.py
(lin_decode: tests/test_gpu_lin_decode.py) reads the inputs back, so it does not depend on how the machine that runs it rounds them, and compares with exact equality.  A new
net is a new entry of SUITES, a design function in the recorder and the tests of what its recordings reach.

A case is (robot, nj, H, nobs, CFSBatch keywords, [run key]), a run key (mode, tier[, noise variant]).  Noise variants of a PSGCFS
run: "full" (12 rows, one per possible iteration), "short" (3 rows: iterations 4.. take the `have == false` branch of prep(2)),
"none".  File names: `<suite>_<case>_in.npy`, `<suite>_<case>_<run key joined by _>.npy`."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 0.1
M200I_X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])
NOISE_ROWS = {"full": 12, "short": 3}
MAX_O_ITER = 12
SOLVE_FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
LIN_FIELDS = ("dist", "grad", "linkid")

BOTH = [("CFS", "default"), ("PSGCFS", "default")]
PLAIN = [("PSGCFS", "default", "full"), ("CFS", "default", "none")]
SUITES = {
    # ---- lin_decode: the work-item decode of the linearisation ---------------------------------------------------------------------
    # The fused solver's linearisation finds the (obstacle, waypoint, link) of a work item e without an integer division:
    # reciprocals computed by the host for the obstacle count and for obstacles x tile width, and one compare per link over the
    # concatenated candidate ranges of the shifted poses (rcp_div; the whole-CU tier keeps the divisions and is pinned here all the
    # same).  Recorded with the runtime divisions and the five-way range chain.  Compared: `dist`, `grad`, `linkid` (the
    # linearisation of x_init through cfs_linearize) and `u`, `x_`, `status`, `iter_O`, `total_iter` (whole solves), 8 problems per
    # shape; both solvers; the default tier and the whole-CU tier; 5x31x7 once with pruning off.  The recorder designs the obstacles
    # with the CPU oracle (link positions, per-link distances) so that links without any candidate, (waypoint, obstacle) pairs with
    # two candidate links, and pairs on the near-zero surrogate of dist_arm all occur, and records the counts per problem.
    #
    # Tile widths (`lin_w`, from the plan of launch_fused_tier; the half-CU tiers w2s / w2m agree, w1 always has one tile here):
    #
    #   case      nj  H  nobs  kernel rows  tiles in the default tier     handle
    #   5x31x7     5  31   7      160        16 + 15 (last shorter)        plain; also run on w1 (one tile of 31) and with pruning off
    #   2x12x1     2  12   1       96        12 (one tile, one obstacle)   plain (two-link arm)
    #   6x40x3     6  40   3      256        14 + 14 + 12 (last shorter)   plain; CFS also on w1 (one tile of 40)
    #   3x20x5     3  20   5       96        20 (one tile)                 plain
    #   5x31x7m    5  31   7      160        11 + 11 + 9 (last shorter)    per-waypoint obstacles (`m` kernels)
    #   5x31x7a    5  31   7      160        16 + 15                       analytic Jacobian (`a` kernels)
    #   5x31x7l    5  31   7      160        16 + 15                       joint position limits (`l` kernels)
    #
    # (5 x 31 x 7 has two static tiles, not three: 17 waypoints fit a tile, and ceil(31 / 2) = 16.  The static handle with three
    # tiles whose last one is shorter -- `rc_tile` and `rc_last` differ, and a third tile starts behind two full ones -- is 6x40x3;
    # 5x31x7m is the same for the per-waypoint kernels.)  Seven obstacles are no power of two and no divisor of the 256 threads, so
    # an item's (obstacle, waypoint, link) changes in every round of every loop.
    "lin_decode": SimpleNamespace(
        B=8, variants=False, fields=LIN_FIELDS + ("u", "x_", "status", "iter_O", "total_iter"), lin_cases=(),
        extra_in=("two_candidates", "surrogate", "idle_links"),
        cases={
            "5x31x7": ("M200i", 5, 31, 7, {}, BOTH + [("CFS", "w1"), ("PSGCFS", "w1")]),
            "2x12x1": ("2L", 2, 12, 1, {}, BOTH),
            "6x40x3": ("M200i", 6, 40, 3, {}, BOTH + [("CFS", "w1")]),
            "3x20x5": ("M200i", 3, 20, 5, {}, BOTH),
            "5x31x7m": ("M200i", 5, 31, 7, dict(obstacles="per_waypoint"), BOTH),
            "5x31x7a": ("M200i", 5, 31, 7, dict(jacobian="analytic"), BOTH),
            "5x31x7l": ("M200i", 5, 31, 7, dict(joint_limits="robot"), BOTH),
        }),
    # ---- wave_balance: the placement of the riding work ----------------------------------------------------------------------------
    # The riding work -- the QP's start vector and the two rollouts it needs, `prep(1..3)` -- runs on the wavefronts that the
    # linearisation phase it rides on leaves with a pass less (launch_fused_tier: FusedParams::ride).  A rollout of joint c is the
    # same two half-wave scans whichever wavefront runs it and the start vector the same expression per element.  Recorded with
    # every prep on wavefronts 0, 1, 2.  Compared: whole solves (SOLVE_FIELDS), 6 problems per run.
    #
    # First wavefront that carries the riding work (0: all four, the mapping from before), from the item counts of tile 0 -- chain
    # `Wc * (2 nj + 1)` (analytic: `Wc`), base distances `nj * Wc * nobs`, minima `Wc * nobs`, `Wc` the tile's waypoints:
    #
    #   case        nj  H  nobs  rows  tile 0   chain / base / minima items   prep(1) / prep(2) / prep(3) start on wavefront
    #   5x30x8       5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (config 3's shape; on w1: old mapping)
    #   5x30x8still  5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (start = goal: the skipped-step branch)
    #   2x12x1       2  12   1    96     12         60 /   24 /  12             1 / 1 / 1     (two joints on six half-waves)
    #   5x31x7       5  31   7   160     16        176 /  560 / 112             3 / 1 / 2     (tile 1 has 15 waypoints: not consulted)
    #   6x40x3       6  40   3   256     14        any                          0 / 0 / 0     (H > 32: one joint per wavefront, unchanged)
    #   5x30x8a      5  30   8   160     15         15 /  600 / 120             1 / 2 / 2     (analytic Jacobian)
    #   5x30x8m      5  30   8   160   narrower    by the plan                  by the counts (per-waypoint obstacles: more tiles)
    #   5x30x8l      5  30   8   160     15        165 /  600 / 120             3 / 2 / 2     (joint position limits)
    #
    # (tests/test_wave_balance_rule.py checks ride_plan below against these rows.)  Only the kernels of the identity Hessian's
    # half-CU tier (w2s: every `PSGCFS default` run) are compiled with the new placement (`CFS_RIDE_IDLE`).  The `CFS default` runs
    # (w2m), the `w1` runs and horizons above 32 execute the mapping from before whatever the table says for their shape: w2m was
    # measured slower with the new placement, w1 was not timed; they are recorded so that they stay pinned if that changes.  The
    # `still` problems start at their goal far from every obstacle (the skipped-step branch of prep(2)): the recorder confirms on
    # the CPU oracle that e_u_all is exactly 0 from some iteration on, and the test asserts the same of the recording.
    "wave_balance": SimpleNamespace(
        B=6, variants=True, fields=SOLVE_FIELDS, lin_cases=(), extra_in=(),
        cases={
            "5x30x8": ("M200i", 5, 30, 8, {}, PLAIN + [("PSGCFS", "default", "short"), ("PSGCFS", "w1", "full"), ("CFS", "w1", "none")]),
            "5x30x8still": ("M200i", 5, 30, 8, {}, [("PSGCFS", "default", "none"), ("PSGCFS", "default", "short")]),
            "2x12x1": ("2L", 2, 12, 1, {}, PLAIN),
            "5x31x7": ("M200i", 5, 31, 7, {}, PLAIN),
            "6x40x3": ("M200i", 6, 40, 3, {}, PLAIN),
            "5x30x8a": ("M200i", 5, 30, 8, dict(jacobian="analytic"), PLAIN),
            "5x30x8m": ("M200i", 5, 30, 8, dict(obstacles="per_waypoint"), PLAIN),
            "5x30x8l": ("M200i", 5, 30, 8, dict(joint_limits="robot"), PLAIN),
        }),
    # ---- fixed_path: what every outer iteration pays whatever its QP does ----------------------------------------------------------
    # In the half-CU tier of the identity Hessian (w2s: the `PSGCFS default` runs) the kinematic chains of the literal linearisation
    # read their operands -- the sin / cos of a joint's variant, the link constants, the capsule points -- ahead of the arithmetic
    # that uses them instead of in dependent LDS round trips (DH robots; the robot's `kind` is read once per tile and the two-link
    # arm keeps fk_step), the kernels of up to 5 joints and 160 rows keep the problem's `ff` in LDS for prep(2) and the cost
    # product, and the post phase (new u, rollout, get_cost, the start vector of the next QP) computes its LDS addresses in place.
    # The CFS (w2m) and whole-CU (w1) runs execute the statements they had and are pinned all the same.  Recorded before the chain
    # phase lost its round trips and `ff` moved on chip, with non-zero `ff`, distinct per problem.  Compared: whole solves
    # (SOLVE_FIELDS), 6 problems per run; for the cases in `lin_cases` also the linearisation of x_init (LIN_FIELDS), which
    # localises a chain error.
    #
    #   case         nj  H  nobs  rows  what it reaches
    #   5x30x8        5  30   8   160   config 3's shape: PSGCFS on the half-CU tier with a noise row per iteration, with 3 rows (`have ==
    #                                   false` in prep(2)) and without noise; CFS (the `x0` branch, `ff` from global memory); both on w1
    #   5x30x8still   5  30   8   160   start = goal far from every obstacle: the skipped-step branch (x_ is the rollout of the unchanged u)
    #   2x12x1        2  12   1    96   the two-link arm: the other `kind` (`t2l` link transforms, which stay on fk_step), a chain of 2 joints
    #   3x30x2        3  30   2    96   the first 3 joints of the M200i: one tile for the whole horizon
    #   5x31x7        5  31   7   160   tiles of 16 + 15: the last tile's Wc != W
    #   6x40x3        6  40   3   256   H > 32: one joint per wavefront in the cost scans, register P columns, `ff` from global memory
    #   5x30x8a       5  30   8   160   analytic Jacobian: the `arm_chain` site
    #   5x30x8m       5  30   8   160   per-waypoint obstacles (MOVE kernels)
    #   5x30x8l       5  30   8   160   joint position limits (LIM kernels)
    #   5x30x8d       5  30   8   160   PSGCFS with `use_weights=False`: the dense QQ product, the other cost branch that reads `ff`
    "fixed_path": SimpleNamespace(
        B=6, variants=True, fields=SOLVE_FIELDS, lin_cases=("2x12x1", "5x31x7", "6x40x3"), extra_in=(),
        cases={
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
        }),
}


def spec(suite, case):
    """what run() and the dtypes need of a case: its tuple by name, the output fields it records, its extra input fields"""
    S = SUITES[suite]
    robot, nj, H, nobs, kw, keys = S.cases[case]
    lin = LIN_FIELDS if case in S.lin_cases else ()                 # on top of what every case of the suite records
    return SimpleNamespace(robot=robot, nj=nj, H=H, nobs=nobs, kw=kw, keys=keys, still=case.endswith("still"),
                           per_waypoint=kw.get("obstacles") == "per_waypoint", fields=S.fields + lin, extra_in=S.extra_in)


def runs(suite, lin_only=False):
    """[(case, mode, tier[, variant])] of a suite; lin_only: the runs that also record the linearisation"""
    return [(case, *key) for case, v in SUITES[suite].cases.items() for key in v[5]
            if not lin_only or "dist" in spec(suite, case).fields]


def golden_path(suite, case, *run_key):
    return os.path.join(GOLDEN, "_".join((suite, case) + (run_key or ("in",))) + ".npy")


def family(pkg, robot, nj, H, still=False):
    """sys_info of a case (weights of tests/test_gpu_tiers.py's single problems), start and goal; still: goal = start"""
    rb = pkg.robotproperty2(robot)
    if robot == "2L":
        x0, xg = np.zeros(2), np.array([np.pi / 2, 0.0])
        kw = dict(Qp=np.diag([10.0, 1.0]), Qv=np.diag([10.0, 1.0]), Rblk=np.diag([5.0, 4.0]), cR=0.1, lim=np.ones(2),
                  max_input_blk=np.ones(2) * 0.25, epsilon_O=1e-6, MAX_O_ITER=MAX_O_ITER)
    else:
        x0 = M200I_X0[:nj]
        xg = x0 * np.array([-1.0, 1, 1, 1, 1, 1])[:nj]
        if still:
            xg = x0.copy()
        kw = dict(Qp=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Qv=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Rblk=np.eye(nj) * 2, cR=50.0,
                  lim=np.ones(nj), max_input_blk=np.ones(nj), epsilon_O=0.1, MAX_O_ITER=MAX_O_ITER)
    return pkg.build_sys_info(rb, nj, H, x0, xg, pkg.line_reference(x0, xg, H), **kw), x0, xg


def in_dtype(nj, H, nobs, per_waypoint=False, extra=(), noise_rows=NOISE_ROWS["full"]):
    oshape = (H, nobs, 6) if per_waypoint else (nobs, 6)
    return [("x_init", "<f8", (2 * H * nj,)), ("xR1", "<f8", (2 * nj,)), ("ff", "<f8", (H * nj,)), ("caug", "<f8"), ("obs", "<f8", oshape),
            ("noise", "<f8", (noise_rows, H * nj))] + [(k, "<i4") for k in extra]


def out_dtype(nj, H, nobs, fields):
    K = MAX_O_ITER
    of = dict(dist=("<f8", (nobs, H)), grad=("<f8", (nobs, H, nj)), linkid=("<i4", (nobs, H)), u=("<f8", (H * nj,)),
              x_=("<f8", (2 * H * nj,)), cost_all=("<f8", (K,)), e_cost_all=("<f8", (K,)), e_u_all=("<f8", (K,)))
    return [(k,) + of.get(k, ("<i4",)) for k in fields]


def dtype_of(suite, case, *run_key):
    """the dtype of golden_path(suite, case, *run_key)"""
    c = spec(suite, case)
    return np.dtype(out_dtype(c.nj, c.H, c.nobs, c.fields) if run_key else in_dtype(c.nj, c.H, c.nobs, c.per_waypoint, c.extra_in))


def noise_of(rec, variant):
    return None if variant == "none" else np.ascontiguousarray(rec["noise"][:, :NOISE_ROWS[variant]])


def run(pkg, spec, mode, tier, variant, rec, no_prune=False, solve=True, linearize=None):
    """the case's handle on the recorded inputs: whole solves and (default: where the case records it) the linearisation of
    x_init, as one record per problem"""
    c = spec
    linearize = "dist" in c.fields if linearize is None else linearize
    s, _, _ = family(pkg, c.robot, c.nj, c.H, c.still)
    n = rec.shape[0]
    h = pkg.CFSBatch(s, c.nobs, np.full(c.nobs, MARGIN), mode=mode, max_batch=n, **c.kw)
    h.debug_options(tier_w1=tier == "w1", no_prune=no_prune)
    arg = {k: np.ascontiguousarray(rec[k]) for k in ("x_init", "xR1", "ff", "caug", "obs")}
    out = np.zeros(n, dtype=out_dtype(c.nj, c.H, c.nobs, c.fields))
    if linearize:
        out["dist"], out["linkid"], out["grad"] = h.linearize(arg["x_init"], arg["obs"])
    if solve:
        r = h.solve(arg["x_init"], arg["xR1"], arg["ff"], arg["caug"], arg["obs"], noise=noise_of(rec, variant) if mode == "PSGCFS" else None)
        for k in c.fields:
            if k not in LIN_FIELDS:
                out[k] = getattr(r, k)
    h.close()
    return out


def differing(got, want, key):
    """indices of the problems whose field `key` is not the same bytes in both records"""
    a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
    n = a.shape[0]
    return np.nonzero((a.reshape(n, -1).view(np.uint8) != b.reshape(n, -1).view(np.uint8)).any(axis=1))[0]


def assert_same_bits(got, want, keys, tag):
    for k in keys:
        bad = differing(got, want, k)
        assert bad.size == 0, f"{tag}: {k} differs from the recording in {bad.size} problems, first {bad[:8].tolist()}"


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
