"""Tool-path audit, CPU: the restatement of tests/path_audit_reference.py against a 16 times denser sampling (both guarantees of the
header), the fixed scene of DESIGN.md section 29, closed forms, every status and state, and the parity inputs' own conditions."""
import math

import numpy as np
import pytest

import ik_reference as IR
import path_audit_reference as PA

ROBOTS = [("M200i", 5), ("M16iB", 6), ("2L", 2)]
INF = math.inf


def _arm(O, name, nj):
    return IR.Arm(O.robotproperty2(name), nj)


def _lim(pkg, name, nj):
    return np.asarray(pkg.robotproperty2(name).thetamax[:nj], float)


@pytest.mark.parametrize("name,nj", ROBOTS)
def test_both_bounds_hold_against_a_denser_sampling(O, pkg, name, nj):
    arm, lim = _arm(O, name, nj), _lim(pkg, name, nj)
    obs, D = PA.two_obstacles(arm, lim)
    rng = np.random.default_rng(5 + nj)
    mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), 0.25 * (lim[:, 1] - lim[:, 0])
    slack_c, slack_e, tight, certified = INF, INF, 0.0, 0
    for step in (0.02, 0.1, 0.3):
        for _ in range(40):
            a = mid + (2 * rng.random(nj) - 1) * half
            d = 2 * rng.random(nj) - 1
            q = np.stack([a, a + step * d / np.abs(d).max()])
            for S in (1, 3, 8):
                r = PA.audit_path(arm, q, obs, D, S)
                PA.check_path(arm.robot, nj, arm.tool, q, S, len(D), r)
                cmin, emax = PA.check_sound(arm, q, obs, D, S, r)
                certified += r.clear_lower > 0
                slack_e = min(slack_e, r.chord_upper - emax)
                if r.clear_lower > 0:                                     # the slack of the guarantee, where there is one
                    slack_c = min(slack_c, cmin - r.clear_lower)
                tight = max(tight, emax / r.chord_upper)
    print(f"[path audit soundness] {name}: least clearance slack of a certified case {slack_c:.3e} m, least chord slack {slack_e:.3e} m, dense e / chord_upper up to "
          f"{tight:.3f}, {certified} of 360 cases certified")
    assert certified > 0 and tight > 0.5                                  # the bounds are exercised, not vacuous


@pytest.mark.parametrize("name,nj", ROBOTS)
def test_the_post_between_two_rows(O, name, nj):
    """both rows clear the post, the motion goes through it: seen at S = 2 and 8, missed by the samples at S = 3, never certified"""
    arm = _arm(O, name, nj)
    q, obs, D = PA.post_scene(arm)
    out = {S: PA.audit_path(arm, q, obs, D, S, min_clearance=0.0) for S in (2, 3, 8)}
    print(f"[path audit post] {name}: rows clear by {out[2].clear_rows:.3f} m; clear_path " + ", ".join(f"S={S}: {r.clear_path:+.3f}" for S, r in out.items())
          + "; clear_lower " + ", ".join(f"S={S}: {r.clear_lower:+.3f}" for S, r in out.items()))
    for S, r in out.items():
        assert r.clear_rows > 0 and r.clear_lower < 0 and r.state_out == 6 and r.status == 0
        assert r.obs_path == 0 and 1 <= r.link_path <= nj
    assert out[2].clear_path < 0 and out[8].clear_path < 0 and out[2].s_path == 0.5 and out[8].s_path == 0.5
    assert out[3].clear_path > 0


@pytest.mark.parametrize("name,nj", ROBOTS)
def test_the_gap_between_sampled_and_certified_closes_with_substeps(O, pkg, name, nj):
    arm, lim = _arm(O, name, nj), _lim(pkg, name, nj)
    obs, D = PA.two_obstacles(arm, lim)
    paths = PA.smooth_paths(lim, 1, 4, 9, seed=3).reshape(4, 9, nj)
    for q in paths:
        r4, r16, r1 = (PA.audit_path(arm, q, obs, D, S) for S in (4, 16, 1))
        for S, r in ((4, r4), (16, r16), (1, r1)):
            PA.check_path(arm.robot, nj, arm.tool, q, S, len(D), r)
            assert r.clear_path - r.clear_lower <= r.L_max / (2 * S) + 1e-12
        assert r16.clear_path - r16.clear_lower < r4.clear_path - r4.clear_lower
        assert r16.chord_upper - r16.chord_err < r4.chord_upper - r4.chord_err
        assert r1.chord_upper == pytest.approx(r1.A_max / 8.0, abs=1e-15) and r1.chord_err == 0.0
        assert r1.clear_rows == r1.clear_path == r4.clear_rows           # S = 1 samples the rows alone


def test_chord_error_of_a_circular_arc(O):
    """rows on a joint-space line through joint 0 of the 2L: the tool point moves on a circle of radius r about the base axis, and
    the same-fraction chord point is farthest from it at the middle of a segment: r (1 - cos(delta/2))"""
    arm = _arm(O, "2L", 2)
    delta, N = 0.3, 5
    q = np.zeros((N, 2))
    q[:, 0] = 0.1 + delta * np.arange(N)
    q[:, 1] = 0.4
    p = arm.pose(q[0])[0] - arm.base
    r = math.hypot(p[0], p[1])
    for S in (2, 8, 64):
        out = PA.audit_path(arm, q, np.zeros((0, 6)), np.zeros(0), S)
        assert abs(out.chord_err - r * (1 - math.cos(delta / 2))) <= 1e-12
        assert out.chord_err <= out.chord_upper <= out.chord_err + out.A_max / (8 * S * S) + 1e-15
    odd = PA.audit_path(arm, q, np.zeros((0, 6)), np.zeros(0), 3)          # no sample at the middle: strictly less, the bound still above
    assert odd.chord_err < r * (1 - math.cos(delta / 2)) <= odd.chord_upper


def test_statuses_states_and_their_order(O, pkg):
    arm, lim = _arm(O, "M200i", 5), _lim(pkg, "M200i", 5)
    obs, D = PA.two_obstacles(arm, lim)
    paths = PA.smooth_paths(lim, 1, 6, 5, seed=9).reshape(6, 5, 5)
    paths[1, 2, 3] = np.nan
    paths[3, 0, 0] = np.inf
    state = np.array([0, 0, 4, 2, 0, 5], np.int32)
    finite = np.isfinite(paths).all(axis=(1, 2))
    off = PA.audit_paths(arm, paths, obs, D, 3, state)
    PA.check_conventions(off, state, finite)
    np.testing.assert_array_equal(off.status, [0, 2, 1, 1, 0, 1])         # a state comes before a non-finite row
    np.testing.assert_array_equal(off.state_out, [0, 3, 4, 2, 0, 5])
    np.testing.assert_array_equal(off.state_out[finite], state[finite])   # thresholds off: state_out == state on finite paths
    # thresholds between the two audited paths' bounds: clearance is tested before the chord
    lo, up = off.clear_lower[[0, 4]], off.chord_upper[[0, 4]]
    both = PA.audit_paths(arm, paths, obs, D, 3, state, min_clearance=lo.max() + 1.0, max_chord=up.min() / 2)
    np.testing.assert_array_equal(both.state_out, [6, 3, 4, 2, 6, 5])
    chord = PA.audit_paths(arm, paths, obs, D, 3, state, min_clearance=lo.min() - 1.0, max_chord=up.min() / 2)
    np.testing.assert_array_equal(chord.state_out, [7, 3, 4, 2, 7, 5])
    if lo[0] != lo[1]:
        one = PA.audit_paths(arm, paths, obs, D, 3, state, min_clearance=lo.mean())
        assert sorted(one.state_out[[0, 4]].tolist()) == [0, 6]
    for r in (both, chord):
        PA.check_conventions(r, state, finite)
    PA.check_state_out(both, lo.max() + 1.0, up.min() / 2)
    PA.check_state_out(chord, lo.min() - 1.0, up.min() / 2)
    np.testing.assert_array_equal(both.status, off.status)


@pytest.mark.parametrize("name,nj", ROBOTS)
def test_two_rows_and_no_obstacles(O, pkg, name, nj):
    arm, lim = _arm(O, name, nj), _lim(pkg, name, nj)
    obs, D = PA.two_obstacles(arm, lim)
    q = PA.smooth_paths(lim, 1, 1, 2, seed=4).reshape(2, nj)
    for S in (1, 5):
        r = PA.audit_path(arm, q, obs, D, S)
        PA.check_path(arm.robot, nj, arm.tool, q, S, 2, r)
        PA.check_sound(arm, q, obs, D, S, r)
        assert r.status == 0 and 0.0 <= r.s_path <= 1.0
        free = PA.audit_path(arm, q, np.zeros((0, 6)), np.zeros(0), S)
        PA.check_path(arm.robot, nj, arm.tool, q, S, 0, free)
        assert free.clear_rows == free.clear_path == free.clear_lower == INF and free.obs_path == -1 and free.link_path == -1 and free.s_path == 0.0
        assert free.chord_err == r.chord_err and free.chord_upper == r.chord_upper and free.state_out == 0
        assert PA.audit_path(arm, q, np.zeros((0, 6)), np.zeros(0), S, min_clearance=1e9).state_out == 0   # +inf clears any threshold


# ---- the parity inputs: what tests/test_gpu_path_audit.py compares the device with ----------------------------------------------------------
@pytest.mark.parametrize("name,nj", ROBOTS + [("M200i", 3), ("M200i", 4)])
def test_parity_inputs_are_well_conditioned(O, pkg, name, nj):
    """prints the movement of every output under a 1e-12 rad change of the rows (DESIGN.md section 29 quotes it), and asserts what the
    GPU comparison relies on: at most 5 % of the audited paths are excluded from the s_path comparison by the gap rule, and no
    state_out decision lies within a factor 2 of its threshold"""
    arm, lim = _arm(O, name, nj), _lim(pkg, name, nj)
    paths, state, obs, D, mc, xc, ref, movement, tol = PA.parity_case(arm, lim)
    print(f"[path audit parity inputs] {name} nj={nj}: min_clearance {mc:.3e}, max_chord {xc:.3e}; movement " + ", ".join(f"{k} {v:.2e}" for k, v in movement.items())
          + f"; tolerance up to {max(tol.values()):.2e}; state_out {np.bincount(ref.state_out, minlength=8).tolist()}")
    ok = ref.status == 0
    PA.check_conventions(ref, state.reshape(-1), np.isfinite(paths).all(axis=(2, 3)).reshape(-1))
    assert ok.sum() >= 12 and (ref.status == 1).any() and (ref.status == 2).any()
    excluded = ok & ~(ref.gap > tol["clear_path"])
    assert excluded.sum() <= 0.05 * ok.sum(), ref.gap[ok]
    lo, up = ref.clear_lower[ok], ref.chord_upper[ok]
    assert ((lo < mc / 2) | (lo > 2 * mc)).all(), lo
    passing = ~(lo < mc)
    assert ((up[passing] < xc / 2) | (up[passing] > 2 * xc)).all(), up
    assert max(tol.values()) <= 1e-6                                      # the comparison stays meaningful
