"""The lin_decode suite of tests/fused_recorded.py (which says why the net exists and what each shape reaches) against its
recordings tests/golden/lin_decode_*.npy: exact equality of `dist`, `grad`, `linkid` (the linearisation of x_init through
cfs_linearize) and of `u`, `x_`, `status`, `iter_O`, `total_iter` (whole solves) in one test per run, 8 problems per shape; 5x31x7
once more with pruning off; and what the recorder's counts and the recorded distances say the obstacles reach.  The other suites
are run by tests/test_gpu_fused_recorded.py, which also checks the layout of these recordings."""
import numpy as np
import pytest

import fused_recorded as R

pytestmark = pytest.mark.gpu
CASES = R.SUITES["lin_decode"].cases


def recording(case, *key):
    return np.load(R.golden_path("lin_decode", case, *key))


@pytest.mark.parametrize("case,mode,tier", R.runs("lin_decode"))
def test_linearisation_and_solve_equal_the_recording(gpu, case, mode, tier):
    want = recording(case, mode, tier)
    got = R.run(gpu, R.spec("lin_decode", case), mode, tier, "full", recording(case))
    R.assert_same_bits(got, want, want.dtype.names, f"{case} {mode} {tier}")


@pytest.mark.parametrize("mode,tier", [("PSGCFS", "default"), ("CFS", "w1")])
def test_unpruned_linearisation_equals_the_recording(gpu, mode, tier):
    """every link at every evaluation point (no candidate lists: the longest concatenated ranges the shifted-pose loop can see)"""
    want = recording("5x31x7", mode, tier)
    got = R.run(gpu, R.spec("lin_decode", "5x31x7"), mode, tier, "full", recording("5x31x7"), no_prune=True, solve=False)
    R.assert_same_bits(got, want, R.LIN_FIELDS, f"5x31x7 {mode} {tier}, pruning off")


@pytest.mark.parametrize("case", list(CASES))
def test_recorded_problems_reach_the_edges(case):
    """what the obstacles were designed for (no device work: the recorder's counts and the recorded distances)"""
    rec = recording(case)
    want = recording(case, "PSGCFS", "default")
    assert rec["two_candidates"].sum() > 0 and rec["surrogate"].sum() > 0
    assert (want["dist"] < 0).any()                        # the surrogate's value is negative (dist_arm_3D_200i_2.m:22-24)
    assert rec["idle_links"].sum() > 0                     # links whose candidate list is empty in every tile
