"""The placement rule of the fused solver's riding work (launch_fused_tier, FusedParams::ride; restated in
tests/fused_recorded.py) and the index arithmetic of the loops that follow it (roll_lds and prep(2) of csrc/cfs_fused.hip),
simulated thread by thread: the chosen wavefronts really have a pass less, and every joint / element is still computed exactly once."""
import numpy as np
import pytest

import fused_recorded as W

FT, WAVE = 256, 64


def passes_per_wavefront(items):
    """passes of `for (e = tid; e < items; e += FT)` that have at least one active lane, per wavefront"""
    tid = np.arange(FT)
    trips = np.maximum(0, -(-(items - tid) // FT))
    return trips.reshape(FT // WAVE, WAVE).max(axis=1)


@pytest.mark.parametrize("items", list(range(0, 1400)) + [20480])
def test_chosen_wavefronts_have_a_pass_less(items):
    first = W.first_free_wavefront(items)
    p = passes_per_wavefront(items)
    if first == 0:
        assert (p == p[0]).all()                           # nobody is free: the mapping from before
    else:
        assert (p[first:] < p[0]).all() and (p[:first] == p[0]).all()


@pytest.mark.parametrize("first", [0, 1, 2, 3])
@pytest.mark.parametrize("nj", [2, 3, 4, 5, 6])
def test_every_joint_is_rolled_once(first, nj):
    """roll_lds, H <= 32: half-wave hw = (tid >> 5) - 2 first rolls joints hw, hw + 2 (4 - first), ..."""
    owners = np.zeros(nj, int)
    for hw in {(tid >> 5) - 2 * first for tid in range(FT)}:
        if hw >= 0:
            owners[hw:nj:2 * (FT // WAVE - first)] += 1
    assert (owners == 1).all()


@pytest.mark.parametrize("first", [0, 1, 2, 3])
@pytest.mark.parametrize("hn", [24, 60, 150, 155, 192, 193])
def test_every_element_of_the_start_vector_is_written_once(first, hn):
    """prep(2): thread tid >= 64 first handles elements tid - 64 first, + (FT - 64 first), ..."""
    owners = np.zeros(hn, int)
    for tid in range(WAVE * first, FT):
        owners[tid - WAVE * first:hn:FT - WAVE * first] += 1
    assert (owners == 1).all()


def test_table_of_the_cases():
    assert W.ride_plan(5, 30, 8, 15) == (3, 2, 2)          # config 3: the rollouts on wavefront 3 / 2-3, the start vector on 2-3
    assert W.ride_plan(2, 12, 1, 12) == (1, 1, 1)
    assert W.ride_plan(5, 31, 7, 16) == (3, 1, 2)
    assert W.ride_plan(6, 40, 3, 14) == (0, 0, 0)          # H > 32: one joint per wavefront, unchanged
    assert W.ride_plan(5, 30, 8, 15, analytic=True) == (1, 2, 2)
    assert W.ride_plan(5, 30, 8, 30) == (2, 3, 0)          # one tile of 30 (whole-CU tier): by the counts; that tier keeps the old mapping
