"""The fused solver returns, bit for bit, what its recordings hold: every run of the suites of tests/fused_recorded.py (which says
why each net exists and what each shape reaches) on the recorded inputs, whole solves and linearisations compared with exact
equality per problem.  The lin_decode suite, whose runs compare solve and linearisation in one test, is run by
tests/test_gpu_lin_decode.py.  The tests without the `gpu` mark need no device: the recordings of all suites have the layout the
module computes, and they reach the branches their problems were designed for."""
import glob
import os

import numpy as np
import pytest

import fused_recorded as R

WAVE, FIXED = R.SUITES["wave_balance"], R.SUITES["fixed_path"]
ALL_RUNS = [(suite, *r) for suite in ("wave_balance", "fixed_path") for r in R.runs(suite)]
LIN_RUNS = [("fixed_path", *r) for r in R.runs("fixed_path", lin_only=True)]


def run_id(run):
    return "-".join(run)


def recording(suite, case, *key):
    return np.load(R.golden_path(suite, case, *key))


@pytest.fixture(scope="module")
def results(gpu):
    """one run per (suite, case, mode, tier[, noise]), shared by the solve and the linearisation comparisons"""
    cache = {}

    def get(suite, case, mode, tier, variant):
        key = (suite, case, mode, tier, variant)
        if key not in cache:
            cache[key] = R.run(gpu, R.spec(suite, case), mode, tier, variant, recording(suite, case))
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("run", ALL_RUNS, ids=run_id)
def test_solve_equals_the_recording(results, run):
    suite, case, *key = run
    want = recording(suite, case, *key)
    R.assert_same_bits(results(*run), want, [k for k in want.dtype.names if k not in R.LIN_FIELDS], " ".join(run))


@pytest.mark.gpu
@pytest.mark.parametrize("run", LIN_RUNS, ids=run_id)
def test_linearisation_equals_the_recording(results, run):
    suite, case, *key = run
    R.assert_same_bits(results(*run), recording(suite, case, *key), R.LIN_FIELDS, " ".join(run) + ", cfs_linearize")


def test_recordings_have_the_layout_of_the_tables():
    """every committed recording of the three suites is one the tables name, holds B problems and has the dtype the module computes"""
    for suite, S in R.SUITES.items():
        named = {R.golden_path(suite, case): (case,) for case in S.cases}
        named.update({R.golden_path(suite, *r): r for r in R.runs(suite)})
        assert set(glob.glob(os.path.join(R.GOLDEN, suite + "_*.npy"))) == set(named)
        for path, (case, *key) in named.items():
            rec = np.load(path)
            assert rec.dtype == R.dtype_of(suite, case, *key), path
            assert rec.shape == (S.B,), path


def test_wave_balance_recordings_reach_the_branches():
    """what the problems were designed for (no device work: the recorded results)"""
    for variant in ("none", "short"):                      # skipped steps: an iteration that left u exactly where it was
        want = recording("wave_balance", "5x30x8still", "PSGCFS", "default", variant)
        skipped = [int((o["e_u_all"][:o["iter_O"] - 1] == 0.0).sum()) for o in want]
        assert sum(n > 0 for n in skipped) >= WAVE.B // 2, skipped
    full, short = (recording("wave_balance", "5x30x8", "PSGCFS", "default", v) for v in ("full", "short"))
    assert (short["iter_O"] - 1 > R.NOISE_ROWS["short"]).all()          # iterations past the last noise row
    assert not np.array_equal(full["u"], short["u"])                    # ... which the missing rows change
    for case, mode, tier, variant in R.runs("wave_balance"):            # every run iterates: prep rides at least twice ...
        if (case, mode) == ("2x12x1", "CFS"):                           # ... but the two-link CFS problems: their first QP is infeasible
            continue                                                    # (status 2 after one linearisation, prep rode once)
        assert (recording("wave_balance", case, mode, tier, variant)["iter_O"] > 2).any(), (case, mode, tier, variant)


def test_fixed_path_recordings_reach_the_branches():
    """what the problems were designed for (no device work: the recorded results)"""
    want = recording("fixed_path", "5x30x8still", "PSGCFS", "default", "none")   # skipped steps: an iteration that left u exactly where it was
    skipped = [int((o["e_u_all"][:o["iter_O"] - 1] == 0.0).sum()) for o in want]
    assert sum(n > 0 for n in skipped) >= FIXED.B // 2, skipped
    full, short = (recording("fixed_path", "5x30x8", "PSGCFS", "default", v) for v in ("full", "short"))
    assert (short["iter_O"] - 1 > R.NOISE_ROWS["short"]).all()          # iterations past the last noise row
    assert not np.array_equal(full["u"], short["u"])                    # ... which the missing rows change
    status = set()
    for case, mode, tier, variant in R.runs("fixed_path"):
        want = recording("fixed_path", case, mode, tier, variant)
        status |= set(want["status"].tolist())
        if (case, mode) == ("2x12x1", "CFS"):                           # the two-link CFS problems: their first QP is infeasible
            continue
        assert (want["iter_O"] > 2).any(), (case, mode, tier, variant)
    assert len(status) > 1, status                                      # status is not uniform across the set
    for case in FIXED.cases:                                            # ff: non-zero, distinct per problem
        ff = recording("fixed_path", case)["ff"]
        assert (np.abs(ff).max(axis=1) > 0).all() and len({f.tobytes() for f in ff}) == FIXED.B, case
