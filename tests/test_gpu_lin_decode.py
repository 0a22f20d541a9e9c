"""The fused solver's linearisation finds the (obstacle, waypoint, link) of a work item without an integer division: reciprocals
computed by the host for the obstacle count and for obstacles x tile width, and one compare per link over the concatenated
candidate ranges of the shifted poses (csrc/cfs_fused.hip, rcp_div; the whole-CU tier keeps the divisions
and is pinned here all the same).  No floating-point statement moved, so
every output must equal, bit for bit, what the kernels with the runtime divisions returned.

The recordings tests/golden/lin_decode_*.npy were written by `tests/tools/record_lin_decode.py` with the library built from the
commit BEFORE the change; the inputs are recorded with them.  Comparisons are exact equality of `dist`, `grad`, `linkid` (the
linearisation of x_init through cfs_linearize) and of `u`, `x_`, `status`, `iter_O`, `total_iter` (whole solves), 8 problems per
shape.  The shapes, the tile width each one gets, and the handles are listed in tests/lin_decode_cases.py: a short last tile with
seven obstacles, one tile with one obstacle, six joints on a 256-row kernel, three joints, per-waypoint obstacles, the analytic
Jacobian, joint limits; both solvers; the default tier and the whole-CU tier; once with pruning off.  The obstacles were chosen
so that links without any candidate, (waypoint, obstacle) pairs with two candidate links, and pairs on the near-zero surrogate of
dist_arm all occur (counted by the recorder with the CPU oracle, asserted below from its record and from the distances)."""
import os

import numpy as np
import pytest

import lin_decode_cases as L

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIN = ("dist", "grad", "linkid")


@pytest.fixture(scope="module")
def inputs():
    return {case: np.load(os.path.join(GOLDEN, f"lin_decode_{case}_in.npy")) for case in L.CASES}


def assert_same_bits(got, want, keys, tag):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        bad = np.nonzero((a.reshape(a.shape[0], -1).view(np.uint8) != b.reshape(b.shape[0], -1).view(np.uint8)).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: {k} differs from the recording in {bad.size} problems, first {bad[:8].tolist()}"


@pytest.mark.parametrize("case,mode,tier", L.RUNS)
def test_linearisation_and_solve_equal_the_recording(gpu, inputs, case, mode, tier):
    rec = inputs[case]
    want = np.load(os.path.join(GOLDEN, f"lin_decode_{case}_{mode}_{tier}.npy"))
    assert rec.shape[0] == want.shape[0] == L.B
    got = L.run(gpu, case, mode, tier, rec)
    assert_same_bits(got, want, want.dtype.names, f"{case} {mode} {tier}")


@pytest.mark.parametrize("mode,tier", [("PSGCFS", "default"), ("CFS", "w1")])
def test_unpruned_linearisation_equals_the_recording(gpu, inputs, mode, tier):
    """every link at every evaluation point (no candidate lists: the longest concatenated ranges the shifted-pose loop can see)"""
    want = np.load(os.path.join(GOLDEN, f"lin_decode_5x31x7_{mode}_{tier}.npy"))
    got = L.run(gpu, "5x31x7", mode, tier, inputs["5x31x7"], no_prune=True, solve=False)
    assert_same_bits(got, want, LIN, f"5x31x7 {mode} {tier}, pruning off")


@pytest.mark.parametrize("case", list(L.CASES))
def test_recorded_problems_reach_the_edges(inputs, case):
    """what the obstacles were designed for (no device work: the recorder's counts and the recorded distances)"""
    rec = inputs[case]
    want = np.load(os.path.join(GOLDEN, f"lin_decode_{case}_PSGCFS_default.npy"))
    assert rec["two_candidates"].sum() > 0 and rec["surrogate"].sum() > 0
    assert (want["dist"] < 0).any()                        # the surrogate's value is negative (dist_arm_3D_200i_2.m:22-24)
    assert rec["idle_links"].sum() > 0                     # links whose candidate list is empty in every tile
