"""The part of the fused solver that every outer iteration pays whatever its QP does (csrc/cfs_fused.hip), in
the half-CU tier of the identity Hessian (w2s: the `PSGCFS default` runs): the kinematic chains of the literal linearisation read
their operands -- the sin / cos of a joint's variant, the link constants, the capsule points -- ahead of the arithmetic that uses
them instead of in dependent LDS round trips (DH robots; the robot's `kind` is read once per tile and the two-link arm keeps
fk_step), the kernels of up to 5 joints and 160 rows keep the problem's `ff` in LDS for prep(2) and the cost product, and the post
phase computes its LDS addresses in place.  No floating-point statement changed, so every output must equal, bit for bit, what the
kernels returned before; the CFS (w2m) and whole-CU (w1) runs execute the statements they had and are pinned all the same.

The recordings tests/golden/fixed_path_*.npy were written by `tests/tools/record_fixed_path.py` with the library built from the
commit BEFORE the change; the inputs are recorded with them (non-zero `ff`, distinct per problem).  Comparisons are exact equality
of whole solves (`u`, `x_`, `cost_all`, `e_cost_all`, `e_u_all`, `iter_O`, `total_iter`, `status`), 6 problems per run, MAX_O_ITER
12; for the two-link arm, 5x31x7 and 6x40x3 also of the linearisation of x_init (`dist`, `grad`, link ids), which localises a chain
error.  The shapes and handles are listed in tests/fixed_path_cases.py."""
import os

import numpy as np
import pytest

import fixed_path_cases as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def inputs():
    return {case: np.load(os.path.join(GOLDEN, f"fixed_path_{case}_in.npy")) for case in F.CASES}


@pytest.fixture(scope="module")
def results(gpu, inputs):
    """one run per (case, mode, tier, noise), shared by the solve and the linearisation comparisons"""
    cache = {}

    def get(case, mode, tier, variant):
        key = (case, mode, tier, variant)
        if key not in cache:
            cache[key] = F.run(gpu, case, mode, tier, variant, inputs[case])
        return cache[key]
    return get


def recording(case, mode, tier, variant):
    return np.load(os.path.join(GOLDEN, f"fixed_path_{case}_{mode}_{tier}_{variant}.npy"))


def differing(got, want, k):
    a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
    return np.nonzero((a.reshape(F.B, -1).view(np.uint8) != b.reshape(F.B, -1).view(np.uint8)).any(axis=1))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode,tier,variant", F.RUNS)
def test_solve_equals_the_recording(results, case, mode, tier, variant):
    want = recording(case, mode, tier, variant)
    got = results(case, mode, tier, variant)
    assert got.shape[0] == want.shape[0] == F.B
    for k in F.OUT_FIELDS:
        bad = differing(got, want, k)
        assert bad.size == 0, f"{case} {mode} {tier} noise {variant}: {k} differs from the recording in problems {bad.tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode,tier,variant", F.LIN_RUNS)
def test_linearisation_equals_the_recording(results, case, mode, tier, variant):
    want = recording(case, mode, tier, variant)
    got = results(case, mode, tier, variant)
    for k in F.LIN_FIELDS:
        bad = differing(got, want, k)
        assert bad.size == 0, f"{case} {mode} {tier}: {k} of cfs_linearize differs from the recording in problems {bad.tolist()}"


def test_recordings_reach_the_branches():
    """what the problems were designed for (no device work: the recorded results)"""
    want = recording("5x30x8still", "PSGCFS", "default", "none")       # skipped steps: an iteration that left u exactly where it was
    skipped = [int((o["e_u_all"][:o["iter_O"] - 1] == 0.0).sum()) for o in want]
    assert sum(n > 0 for n in skipped) >= F.B // 2, skipped
    full, short = recording("5x30x8", "PSGCFS", "default", "full"), recording("5x30x8", "PSGCFS", "default", "short")
    assert (short["iter_O"] - 1 > F.NOISE_ROWS["short"]).all()          # iterations past the last noise row
    assert not np.array_equal(full["u"], short["u"])                    # ... which the missing rows change
    status = set()
    for case, mode, tier, variant in F.RUNS:
        want = recording(case, mode, tier, variant)
        status |= set(want["status"].tolist())
        if (case, mode) == ("2x12x1", "CFS"):                           # the two-link CFS problems: their first QP is infeasible
            continue
        assert (want["iter_O"] > 2).any(), (case, mode, tier, variant)
    assert len(status) > 1, status                                      # status is not uniform across the set
    for case in F.CASES:                                                # ff: non-zero, distinct per problem
        ff = np.load(os.path.join(GOLDEN, f"fixed_path_{case}_in.npy"))["ff"]
        assert (np.abs(ff).max(axis=1) > 0).all() and len({f.tobytes() for f in ff}) == F.B, case
