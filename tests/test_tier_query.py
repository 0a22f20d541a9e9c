"""cfs_debug_fused_tier (include/cfs_hip.h): which tier of the fused solver a shape runs, answered on the host by the rule
launch_fused itself reads.  It is what makes a GPU test of the w1 tier meaningful: a comparison of "default" against "forced w1" proves
nothing when both ran the same kernels.  No device is touched (CPU)."""
import ctypes as C
import itertools
import os
import re

import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import solvers
from motionplanning_5d_m_amd.solvers import fused_tier

from tier_shapes import BATCH_SHAPES, DEFAULT_W1_NJ_H, DEFAULT_W1_NOBS, SINGLE_SHAPES, instantiation

W1, W2M, W2S = 0, 1, 2


def _header_define(name):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfs_hip.h")).read()
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)", src, flags=re.M).group(1))


MAX_H, MAX_OBS = _header_define("CFS_MAX_H"), _header_define("CFS_MAX_OBS")
MODES = ("CFS", "PSGCFS")


def _tier_or_none(*a, **kw):
    try:
        return fused_tier(*a, **kw)
    except pkg.CfsError as e:
        assert e.code == -1
        return None


def _sweep():
    """a grid over the admissible shapes: every joint count, horizons around the 96 / 160 / 256-row thresholds, obstacle counts to the cap"""
    for nj in range(2, 7):
        hs = {1, 3, 16, 30, 40, 50, MAX_H} | {h for q in (96, 160) for h in (q // nj, q // nj + 1) if 1 <= h <= MAX_H}
        for H in sorted(hs):
            for nobs in (1, 2, 3, 4, 6, 8, 12, 16, 24, MAX_OBS):
                yield nj, H, nobs


def test_tier_names():
    assert solvers.FUSED_TIERS == ("w1", "w2m", "w2s")


def test_each_solver_has_its_own_half_cu_tier_and_force_w1_wins():
    seen = set()
    for nj, H, nobs in _sweep():
        c, p = _tier_or_none(nj, H, nobs, "CFS"), _tier_or_none(nj, H, nobs, "PSGCFS")
        assert (c is None) == (p is None)                 # creation is refused by the w1 plan, which does not depend on the solver
        if c is None:
            continue
        assert c in (W1, W2M) and p in (W1, W2S), (nj, H, nobs, c, p)
        seen |= {("CFS", c), ("PSGCFS", p)}
        for mode in MODES:
            assert fused_tier(nj, H, nobs, mode, force_w1=True) == W1
    assert seen == {("CFS", W1), ("CFS", W2M), ("PSGCFS", W1), ("PSGCFS", W2S)}     # the sweep reaches every answer


def test_shapes_for_gpu_tier_tests_run_a_half_cu_tier_by_default():
    for tag, (nj, H, nobs, modes) in BATCH_SHAPES.items():
        for mode in modes:
            assert fused_tier(nj, H, nobs, mode) == (W2M if mode == "CFS" else W2S), (tag, mode)
            assert fused_tier(nj, H, nobs, mode, force_w1=True) == W1
    for (_, nj, H), inst in SINGLE_SHAPES.items():
        assert instantiation(nj, H) == inst
        assert fused_tier(nj, H, 1, "CFS") == W2M and fused_tier(nj, H, 1, "PSGCFS") == W2S, (nj, H)
    # the variant tests (soft QP, limits, per-waypoint obstacles, analytic Jacobian) run config 3: nj 5, H 30, 8 obstacles
    assert fused_tier(5, 30, 8, "CFS") == W2M and fused_tier(5, 30, 8, "PSGCFS") == W2S


def test_a_160_row_shape_reaches_w1_by_default():
    """nj 5, H 30 (nn = 150, the 160-row kernels): the smallest obstacle count that no longer fits half a CU, per solver -- the
    shapes to solve on w1 with no debug flag.  w2s keeps 16 inverse-Gram columns in LDS, so PSGCFS leaves half a CU first."""
    nj, H = DEFAULT_W1_NJ_H
    assert nj * H <= 160
    assert DEFAULT_W1_NOBS == {"CFS": 25, "PSGCFS": 13}
    for mode in MODES:
        tiers = [_tier_or_none(nj, H, n, mode) for n in range(1, MAX_OBS + 1)]
        assert 1 + next(i for i, t in enumerate(tiers) if t == W1) == DEFAULT_W1_NOBS[mode], (mode, tiers)
        assert fused_tier(nj, H, DEFAULT_W1_NOBS[mode] - 1, mode) != W1 and fused_tier(nj, H, DEFAULT_W1_NOBS[mode], mode) == W1


def test_tier_is_monotone_in_the_obstacle_count():
    """more obstacles never move a shape back to a half-CU tier, and once creation is refused it stays refused"""
    for nj in range(2, 7):
        for H in (1, 8, 16, 24, 30, 40, 50, MAX_H):
            for mode in MODES:
                tiers = [_tier_or_none(nj, H, n, mode) for n in range(1, MAX_OBS + 1)]
                state = 0                                 # 0 half-CU, 1 w1, 2 refused
                for n, t in enumerate(tiers, 1):
                    now = 2 if t is None else (1 if t == W1 else 0)
                    assert now >= state, (nj, H, mode, n, tiers)
                    state = now


def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = pkg.lib()
    good = dict(nj=5, H=30, nobs=8, mode=0, pw=0, lim=0, force=0)
    bad = [dict(nj=1), dict(nj=7), dict(nj=0), dict(H=0), dict(H=MAX_H + 1), dict(H=-3), dict(nobs=0), dict(nobs=MAX_OBS + 1),
           dict(mode=2), dict(mode=-1),
           dict(nj=5, H=MAX_H, nobs=MAX_OBS)]             # the shape test_abi.py's budget test creates in vain
    for change in bad:
        a = dict(good, **change)
        t = C.c_int(-77)
        rc = lib.cfs_debug_fused_tier(a["nj"], a["H"], a["nobs"], a["mode"], a["pw"], a["lim"], a["force"], C.byref(t))
        assert rc == -1 and t.value == -77, change
        assert lib.cfs_last_error()                       # the usual message
    assert lib.cfs_debug_fused_tier(5, 30, 8, 0, 0, 0, 0, None) == -1
    assert b"NULL" in lib.cfs_last_error()
    t = C.c_int(-77)
    assert lib.cfs_debug_fused_tier(5, 30, 8, 0, 0, 0, 0, C.byref(t)) == 0 and t.value == W2M
    with pytest.raises(pkg.CfsError) as e:
        fused_tier(5, MAX_H, MAX_OBS)
    assert e.value.code == -1 and "on-chip budget" in str(e.value)
    with pytest.raises(KeyError):
        fused_tier(5, 30, 8, "CHOMP")


def test_per_waypoint_and_limited_handles_run_the_static_tier_or_are_refused():
    """the rule of fused_keeps_tier: a variant handle never changes the tier of its shape"""
    refused = same = 0
    for (nj, H, nobs), mode in itertools.product(_sweep(), MODES):
        plain = _tier_or_none(nj, H, nobs, mode)
        for pw, lim in ((True, False), (False, True), (True, True)):
            t = _tier_or_none(nj, H, nobs, mode, per_waypoint=pw, limits=lim)
            if plain is None:
                assert t is None
            elif t is None:
                refused += 1
            else:
                assert t == plain, (nj, H, nobs, mode, pw, lim)
                same += 1
                assert fused_tier(nj, H, nobs, mode, per_waypoint=pw, limits=lim, force_w1=True) == W1
    assert same > 0
    print(f"variant shapes: {same} run the static tier, {refused} refused")
