"""The fused solver's riding work -- the QP's start vector and the two rollouts it needs, `prep(1..3)` of csrc/cfs_fused.hip -- runs on
the wavefronts that the linearisation phase it rides on leaves with a pass less (launch_fused_tier: FusedParams::ride; DESIGN.md
section 4.1).  Only the half-CU tier of the identity Hessian (w2s: the `PSGCFS default` runs) is compiled that way; the CFS tier
(w2m: the `CFS default` runs), the whole-CU tier (`w1`) and horizons above 32 keep the mapping from before and are pinned here all
the same.  A rollout of
joint c is the same two half-wave scans whichever wavefront runs it and the start vector the same expression per element, so every
output must equal, bit for bit, what the kernels returned with everything on wavefronts 0, 1, 2.

The recordings tests/golden/wave_balance_*.npy were written by `tests/tools/record_wave_balance.py` with the library built from
the commit BEFORE the change; the inputs are recorded with them.  Comparisons are exact equality of whole solves (`u`, `x_`,
`cost_all`, `e_cost_all`, `e_u_all`, `iter_O`, `total_iter`, `status`), 6 problems per run.  The shapes, the wavefront each prep
starts on, and the handles are listed in tests/wave_balance_cases.py: config 3's shape with PSGCFS and a noise row per iteration,
with fewer noise rows than iterations (`have == false`), with CFS (the `x0` branch) and on the whole-CU tier; start equal to goal
far from every obstacle (the skipped-step branch of prep(2): the recorder confirms on the CPU oracle that e_u_all is exactly 0 from
some iteration on, and the recording shows the same below); two joints; a short last tile; six joints with H = 40 on the 256-row
kernel; an analytic, a per-waypoint-obstacle and a joint-limit handle."""
import os

import numpy as np
import pytest

import wave_balance_cases as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def inputs():
    return {case: np.load(os.path.join(GOLDEN, f"wave_balance_{case}_in.npy")) for case in W.CASES}


def recording(case, mode, tier, variant):
    return np.load(os.path.join(GOLDEN, f"wave_balance_{case}_{mode}_{tier}_{variant}.npy"))


@pytest.mark.parametrize("case,mode,tier,variant", W.RUNS)
def test_solve_equals_the_recording(gpu, inputs, case, mode, tier, variant):
    rec, want = inputs[case], recording(case, mode, tier, variant)
    assert rec.shape[0] == want.shape[0] == W.B
    got = W.run(gpu, case, mode, tier, variant, rec)
    for k in W.OUT_FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        bad = np.nonzero((a.reshape(W.B, -1).view(np.uint8) != b.reshape(W.B, -1).view(np.uint8)).any(axis=1))[0]
        assert bad.size == 0, f"{case} {mode} {tier} noise {variant}: {k} differs from the recording in problems {bad.tolist()}"


def test_recordings_reach_the_branches():
    """what the problems were designed for (no device work: the recorded results)"""
    for variant in ("none", "short"):                      # skipped steps: an iteration that left u exactly where it was
        want = recording("5x30x8still", "PSGCFS", "default", variant)
        skipped = [int((o["e_u_all"][:o["iter_O"] - 1] == 0.0).sum()) for o in want]
        assert sum(n > 0 for n in skipped) >= W.B // 2, skipped
    full, short = recording("5x30x8", "PSGCFS", "default", "full"), recording("5x30x8", "PSGCFS", "default", "short")
    assert (short["iter_O"] - 1 > W.NOISE_ROWS["short"]).all()          # iterations past the last noise row
    assert not np.array_equal(full["u"], short["u"])                    # ... which the missing rows change
    for case in W.CASES:                                                # every run iterates: prep rides at least twice ...
        for mode, tier, variant in W.CASES[case][5]:
            if (case, mode) == ("2x12x1", "CFS"):                       # ... but the two-link CFS problems: their first QP is infeasible
                continue                                                # (status 2 after one linearisation, prep rode once)
            assert (recording(case, mode, tier, variant)["iter_O"] > 2).any(), (case, mode, tier, variant)
