"""The CPU restatement of the path-timing contract (tests/path_time_reference.py) against what the contract promises: a closed-form
trapezoid, the limits, no slack, exact scaling, the stop rows, every status, the selection, and how far a 1e-12 rad change of the
rows moves the answer (the figure DESIGN.md section 28 quotes).  No device (CPU)."""
import numpy as np
import pytest

import path_time_reference as PT

LIMS = {2: np.array([[-3.0, 3.0]] * 2), 5: np.array([[-2.5, 2.5]] * 5), 6: np.array([[-2.0, 2.0]] * 6)}


def fake_points(q):
    """a smooth nonlinear map of the first two joints and the sum of all: any tool point serves the restatement"""
    a, b = q[..., 0], q[..., 0] + q[..., 1]
    return np.stack([np.cos(a) + 0.5 * np.cos(b), np.sin(a) + 0.5 * np.sin(b), 0.1 * q.sum(axis=-1)], axis=-1)


def _line():
    q = (0.1 * np.arange(17))[:, None]
    return q, np.array([0.1 * np.sqrt(32.0)]), np.array([0.4])


def test_trapezoid_matches_the_closed_form():
    q, v, a = _line()
    r = PT.time_path(q, v, a)
    assert r.status == 0
    # 0.1 * n is not a binary fraction, so the rows are 0.1 apart to a rounding and b rises by 8 per row to a few of them
    np.testing.assert_allclose(r.b[:5], [0.0, 8.0, 16.0, 24.0, 32.0], rtol=1e-13, atol=0)
    np.testing.assert_allclose(r.b[-5:], [32.0, 24.0, 16.0, 8.0, 0.0], rtol=1e-13, atol=0)
    np.testing.assert_allclose(r.b[4:13], 32.0, rtol=1e-13)
    L = 1.6
    assert abs(r.duration - (L / v[0] + v[0] / a[0])) <= 1e-12


def test_trapezoid_under_a_binding_feed():
    q, v, a = _line()
    pts = np.concatenate([0.5 * q, np.zeros((17, 2))], axis=1)          # 0.05 m per row; feed 0.2 m/s: sdot <= 4 < sqrt(32)
    r = PT.time_path(q, v, a, feed=0.2, points=pts)
    assert r.status == 0
    np.testing.assert_allclose(r.b[2:15], 16.0, rtol=1e-13)
    assert abs(r.duration - (16.0 / 4.0 + 4.0 / 4.0)) <= 1e-12          # 16 rows at sdot 4, ramps of sdot' = ubar = 4
    acc, vel, fd = PT.limit_ratios(q, r.sdot, v, a, 0.2, pts)
    assert fd <= 1.0 + 1e-12 and vel < 0.8


CASES = [(nj, N, feed, k) for nj in (2, 5, 6) for N in (3, 4, 17, 257) for feed in (PT.INF, 0.3) for k in (0, 8)]


@pytest.mark.parametrize("nj,N,feed,k", CASES)
def test_limits_hold_and_no_row_has_slack(nj, N, feed, k):
    paths = PT.smooth_paths(LIMS[nj], 2, 3, N, seed=100 * nj + N)
    vmax, amax = np.linspace(0.8, 1.6, nj), np.linspace(3.0, 1.5, nj)
    for q in paths.reshape(-1, N, nj):
        pts = fake_points(q)
        r = PT.time_path(q, vmax, amax, feed, pts, 0.5, k)
        assert r.status == 0 and (r.b[~PT.stop_rows(N, k)] > 0).all() and (r.b[PT.stop_rows(N, k)] == 0).all()
        acc, vel, fd = PT.limit_ratios(q, r.sdot, vmax, amax, feed, pts)
        assert acc <= 1.0 + 1e-12 and vel <= 1.0 + 1e-12 and fd <= 1.0 + 1e-12
        assert (PT.slack(q, r.sdot, vmax, amax, feed, pts, 0.5, k, b=r.b) == 0.0).all()
        assert r.time[0] == 0.0 and (np.diff(r.time) > 0).all() and r.duration == r.time[-1]


@pytest.mark.parametrize("feed", [PT.INF, 0.3])
def test_scaling_the_limits_halves_every_time_stamp_bit_for_bit(feed):
    nj, N = 5, 33
    vmax, amax = np.linspace(0.8, 1.6, nj), np.linspace(3.0, 1.5, nj)
    for q in PT.smooth_paths(LIMS[nj], 1, 4, N, seed=5)[0]:
        pts = fake_points(q)
        r1 = PT.time_path(q, vmax, amax, feed, pts, 0.5, 8)
        r2 = PT.time_path(q, 2 * vmax, 4 * amax, 2 * feed, pts, 0.5, 8)
        assert r1.status == 0 and r2.status == 0
        np.testing.assert_array_equal(r2.time, r1.time / 2)
        np.testing.assert_array_equal(r2.sdot, r1.sdot * 2)


def test_corners_rest_exactly_at_the_multiples_of_k():
    nj, k, N = 5, 4, 13
    q = PT.smooth_paths(LIMS[nj], 1, 1, N, seed=9)[0, 0]
    r = PT.time_path(q, np.ones(nj), 2 * np.ones(nj), stop_every=k)
    stops = np.arange(N) % k == 0
    assert r.status == 0 and (r.sdot[stops] == 0.0).all() and (r.sdot[~stops] > 0).all()


def test_every_status():
    nj = 5
    q = PT.smooth_paths(LIMS[nj], 1, 1, 9, seed=3)[0, 0]
    one = np.ones(nj)
    assert PT.time_path(q, one, one).status == 0
    assert PT.time_path(q, one, one, state=2).status == 1
    bad = q.copy(); bad[4, 2] = np.nan
    assert PT.time_path(bad, one, one).status == 2
    bad = q.copy(); bad[4, 2] = np.inf
    assert PT.time_path(bad, one, one).status == 2
    assert PT.time_path(q[:4], one, one, stop_every=2).status == 3      # rows 0, 2 and 3 rest: 2 and 3 are neighbours
    rep = q.copy(); rep[5] = rep[4]
    r = PT.time_path(rep, one, one)
    assert r.status == 4 and np.isnan(r.time).all() and np.isnan(r.sdot).all() and np.isnan(r.duration)
    rep[4, 0] = np.nan                                                  # the first status that applies
    assert PT.time_path(rep, one, one).status == 2
    assert PT.time_path(rep, one, one, state=1).status == 1


def test_selection_prefers_the_lowest_index_on_a_tie():
    nj, N = 2, 9
    p = PT.smooth_paths(LIMS[nj], 2, 4, N, seed=1)
    p[0, 1] = p[0, 3] = p[0, 0]                                         # three equal paths, then a longer one made slower
    p[0, 2] = p[0, 0] * 1.5
    state = np.zeros((2, 4), int); state[1] = 7
    r = PT.time_paths(p, np.ones(nj), np.ones(nj), state=state)
    assert r.duration[0, 0] == r.duration[0, 1] == r.duration[0, 3] < r.duration[0, 2]
    assert r.selected.tolist() == [0, -1] and r.group_status.tolist() == [0, 1]
    state[0, 0] = 1
    r = PT.time_paths(p, np.ones(nj), np.ones(nj), state=state)
    assert r.selected.tolist() == [1, -1]


@pytest.mark.parametrize("name,nj", [("M200i", 5), ("M16iB", 6), ("2L", 2)])
def test_a_1e_12_change_of_the_rows_changes_no_status(O, pkg, name, nj, capsys):
    """parity_case asserts that no status changes; the movement printed here is the figure of DESIGN.md section 28"""
    import ik_reference as R
    robot = O.robotproperty2(name)
    arm = R.Arm(robot, nj)
    lim = np.asarray(pkg.robotproperty2(name).thetamax, float)[:nj]
    for k in (0, 4):                                                    # the two settings the device is compared on
        _, _, out = PT.parity_case(arm, lim, k)
        for with_feed, (ref, movement, tol) in out.items():
            with capsys.disabled():
                print(f"\n[path timing] {name} feed={with_feed} stops every {k}: a {PT.PARITY['kick']:g} rad change of every row moves a time "
                      f"stamp or sdot by at most {movement:.3e} (durations {ref.duration.min():.3f}..{ref.duration.max():.3f} s)")
            assert movement < 1e-6 and tol >= 1e-10
