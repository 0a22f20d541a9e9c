"""The analytic Jacobian mode (cfs_problem_set_jacobian(CFS_JAC_ANALYTIC), cfs_dist_arm_grad; include/cfs_hip.h).

1. cfs_dist_arm_grad is the exact derivative of the active branch of dist_arm: against the oracle's dist_arm differentiated
   per joint with derivest (DERIVESTsuite) on random poses of all three robot kinds, against a tiny central difference on
   near-zero-surrogate poses, and against the literal num_jac to O(eps) on smooth poses; d and linkid are cfs_dist_arm's.
2. One code path: cfs_linearize on an analytic handle returns cfs_dist_arm_grad's numbers bit for bit, and cfs_get_con
   builds its rows from them.
3. The whole solve runs the analytic linearisation at every outer iteration: each logged iterate is one oracle QP on the
   rows cfs_get_con (analytic) builds at the device's previous iterate.
4. The default is untouched: fd_literal handles -- fresh, explicit, or switched back from analytic -- give bit-identical
   solves, and mesh rows are the same in both modes.
5. End to end against the literal mode (the bounds are stated and justified at each test).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROBOTS = (("M200i", 5, [2.35, 7.7, 0.0], [3.95, 9.3, 1.4]), ("M16iB", 5, [2.45, 7.7, 0.0], [4.05, 9.3, 1.6]),
          ("2L", 2, [-0.55, -0.55, 0.0], [0.55, 0.55, 0.0]))


def _random_case(rng, lo, hi, nj, N, nobs):
    th = rng.uniform(-2.0, 2.0, (N, nj))
    obs = rng.uniform(lo + lo, hi + hi, (nobs, 6))
    obs[-1, 3:] = obs[-1, :3]                                       # a zero-length obstacle (the 2L point obstacle)
    if lo[2] == hi[2]:
        obs[:, 2] = obs[:, 5] = 0.0                                 # the 2L arm moves in z = 0
    return th, obs


# ---- 1. the gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,nj,lo,hi", ROBOTS)
def test_gradient_against_derivest(gpu, O, rid, nj, lo, hi):
    rng = np.random.default_rng(5)
    robot, orobot = gpu.robotproperty2(rid), O.robotproperty2(rid)
    th, obs = _random_case(rng, lo, hi, nj, 48, 4)
    d, lid, g = gpu.dist_arm(robot, th, obs, want_grad=True)
    d0, lid0 = gpu.dist_arm(robot, th, obs)
    np.testing.assert_array_equal(d, d0)                            # the distances and links are cfs_dist_arm's, bit for bit
    np.testing.assert_array_equal(lid, lid0)
    assert g.shape == (48, 4, nj)
    checked, worst, n_all = 0, 0.0, 0
    for n in range(th.shape[0]):
        for j in range(obs.shape[0]):
            ol = np.stack([obs[j, :3], obs[j, 3:]], axis=1)
            for m in range(nj):
                n_all += 1
                if m >= lid[n, j]:                                   # joints beyond the winning link do not move it
                    assert g[n, j, m] == 0.0
                def f(x, n=n, m=m, ol=ol):
                    t = th[n].copy(); t[m] = x
                    return O.dist_arm(orobot, t, ol)[0]
                # no kink near the pose: the same link and branch (sign of d) at +-1e-3 along joint m
                near = []
                for h in (-1e-3, 1e-3):
                    t = th[n].copy(); t[m] += h
                    near.append(O.dist_arm(orobot, t, ol))
                if any(l2 != lid[n, j] or (dd < 1e-4) != (d[n, j] < 1e-4) for dd, l2 in near):
                    continue
                der, err = O.derivest(f, th[n, m])
                # derivest's widest steps (MaxStep 100 rad) span whole periods of the arm: on a few smooth poses it returns
                # (0, 0); its answer is used where its error estimate is small AND it agrees with a 1e-5 central difference
                cd = (f(th[n, m] + 1e-5) - f(th[n, m] - 1e-5)) / 2e-5
                if not (err < 1e-9 and abs(der - cd) < 1e-5):
                    continue
                checked += 1
                worst = max(worst, abs(der - g[n, j, m]))
                assert abs(der - g[n, j, m]) < 1e-8, (rid, n, j, m, der, g[n, j, m], err)
    print(f"[{rid}] {checked} of {n_all} (pose, obstacle, joint) derivatives checked against derivest: max |diff| {worst:.2e}")
    assert checked >= 0.5 * n_all                                   # measured: M200i 958 / 960 (max 4.6e-12), M16iB 958 / 960 (4.0e-11), 2L 379 / 384 (6.2e-13)


def test_gradient_on_the_surrogate_branch_and_clamps(gpu, O):
    # 2L: a point obstacle ON link 2 -- near-zero surrogate dis = -|c - p1e|, c the obstacle's projection (dist_arm_2L.m:15-17)
    r2, o2 = gpu.robotproperty2("2L"), O.robotproperty2("2L")
    th = np.array([[0.3, -0.4], [1.1, 0.7]])
    obs = []
    for t0, t1 in th:
        p = np.array([0.3 * np.cos(t0), 0.3 * np.sin(t0), 0.0])
        q = p + 0.08 * np.array([np.cos(t0 + t1), np.sin(t0 + t1), 0.0])
        obs.append(np.concatenate([q, q]))
    for n in range(2):
        d, lid, g = gpu.dist_arm(r2, th[n:n + 1], obs[n][None], want_grad=True)
        assert d[0, 0] < 0 and lid[0, 0] == 2                      # the surrogate branch won
        ol = np.stack([obs[n][:3], obs[n][3:]], axis=1)
        for m in range(2):
            h = 1e-7                                                 # moves the arm by < 1e-7: the branch is kept
            tp, tm = th[n].copy(), th[n].copy(); tp[m] += h; tm[m] -= h
            fp, fm = O.dist_arm(o2, tp, ol)[0], O.dist_arm(o2, tm, ol)[0]
            assert fp < 0 and fm < 0
            assert abs((fp - fm) / (2 * h) - g[0, 0, m]) < 1e-6, (n, m, (fp - fm) / (2 * h), g[0, 0, m])
    # M200i: an obstacle segment crossing the axis of link 4 (the 3-D surrogate)
    rb, orb = gpu.robotproperty2("M200i"), O.robotproperty2("M200i")
    t = np.array([[0.4, 0.3, -0.2, 0.5, -0.7]])
    _, _, pos = gpu.dist_arm(rb, t, np.zeros((1, 6)), want_pos=True)
    c = 0.3 * pos[0, 3, 0] + 0.7 * pos[0, 3, 1]                     # a point inside link 4's axis
    ob = np.concatenate([c + [0.0, 0.0, 0.2], c - [0.0, 0.0, 0.2]])[None]
    d, lid, g = gpu.dist_arm(rb, t, ob, want_grad=True)
    assert d[0, 0] < 0 and lid[0, 0] == 4
    ol = np.stack([ob[0, :3], ob[0, 3:]], axis=1)
    for m in range(5):
        h = 1e-7
        tp, tm = t[0].copy(), t[0].copy(); tp[m] += h; tm[m] -= h
        fp, fm = O.dist_arm(orb, tp, ol)[0], O.dist_arm(orb, tm, ol)[0]
        assert fp < 0 and fm < 0
        assert abs((fp - fm) / (2 * h) - g[0, 0, m]) < 1e-6, (m, (fp - fm) / (2 * h), g[0, 0, m])
    # a clamp: point obstacle beyond the end of link 2 (t = 1 clamped): d = |p_end - o|, the clamped t contributes nothing
    o = np.array([0.7, 0.1, 0.0])
    d, lid, g = gpu.dist_arm(r2, np.zeros((1, 2)), np.concatenate([o, o])[None], want_grad=True)
    e = np.array([0.5, 0.0, 0.0]) - o
    assert lid[0, 0] == 2 and abs(d[0, 0] - np.linalg.norm(e)) < 1e-15
    want = [e @ np.array([0.0, 0.5, 0.0]) / np.linalg.norm(e), e @ np.array([0.0, 0.2, 0.0]) / np.linalg.norm(e)]
    np.testing.assert_allclose(g[0, 0], want, rtol=0, atol=1e-15)


def test_gradient_against_the_literal_num_jac(gpu, c3):
    """On smooth poses (the same link at every num_jac evaluation point and no surrogate) the literal central difference is
    the derivative to O(eps^2) plus its rounding, eps = 1e-5, and num_jac's un-restored xp shifts the later joints' stencils
    by eps/2: agreement to 1e-4.  Measured on 15 356 of 15 360 entries: max 6.5e-5, median 1.4e-6."""
    s, bt = c3
    idx = np.arange(64)
    fd = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode="CFS", max_batch=64)
    an = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode="CFS", max_batch=64, jacobian="analytic")
    d_f, l_f, g_f = fd.linearize(bt.x_init[idx], bt.obs[idx])
    d_a, l_a, g_a = an.linearize(bt.x_init[idx], bt.obs[idx])
    np.testing.assert_array_equal(d_f, d_a)                         # same base-pose distances and links, bit for bit
    np.testing.assert_array_equal(l_f, l_a)
    H, nj = s.H, 5
    th = bt.x_init[idx].reshape(64, H, 2 * nj)[:, :, :nj]
    smooth = np.ones_like(d_f, bool)
    for m in range(nj):
        for sg in (-1, 1):
            t = th.copy(); t[:, :, m] += sg * 1e-5
            for b in range(64):
                dd, ll = gpu.dist_arm(s.robot, t[b], bt.obs[b])
                smooth[b] &= (ll.T == l_f[b]) & (dd.T > 1e-3)
    smooth &= d_f > 1e-3
    diff = np.abs(g_f - g_a).max(axis=-1)
    print(f"literal num_jac vs analytic on {int(smooth.sum())} of {smooth.size} smooth (problem, obstacle, waypoint): "
          f"max {diff[smooth].max():.2e}, median {np.median(diff[smooth]):.2e}; on the rest max {diff[~smooth].max() if (~smooth).any() else 0:.2e}")
    assert smooth.sum() >= 0.5 * smooth.size
    assert diff[smooth].max() < 1e-4
    assert fd.jacobian == "fd_literal" and an.jacobian == "analytic"
    fd.close(); an.close()


# ---- 2. one code path ---------------------------------------------------------------------------------------------------
def test_linearize_and_get_con_use_the_same_code(gpu, c3):
    s, bt = c3
    B, H, nj = 32, s.H, 5
    an = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode="CFS", max_batch=B, jacobian="analytic")
    x_ = bt.x_init[:B].copy()
    x_[:, :] += 0.05 * np.random.default_rng(3).standard_normal(x_.shape)   # not only the initial lines
    dist, lid, grad = an.linearize(x_, bt.obs[:B])
    th = x_.reshape(B, H, 2 * nj)[:, :, :nj]
    for b in range(B):
        d1, l1, g1 = gpu.dist_arm(s.robot, th[b], bt.obs[b], want_grad=True)
        np.testing.assert_array_equal(dist[b], d1.T)
        np.testing.assert_array_equal(lid[b], l1.T)
        np.testing.assert_array_equal(grad[b], g1.transpose(1, 0, 2))
    # get_con's collision rows: -(Diff' * Bpos block) built from exactly this grad, binq = d - margin at u = 0
    A, bq = an.get_con(x_, np.zeros((B, H * nj)), bt.xR1[:B], bt.obs[:B])
    per, dt = 1 + 2 * nj, s.robot.delta_t
    rows = np.arange(bt.nobs * H) * per
    for b in range(4):
        Ac = A[b][rows].reshape(bt.nobs, H, H, nj)                  # (j, i, k, c)
        for i in (0, H // 2, H - 1):
            for k in range(H):
                want = -(grad[b][:, i, :] * ((i - k) + 0.5) * dt * dt) if k <= i else np.zeros((bt.nobs, nj))
                np.testing.assert_array_equal(Ac[:, i, k, :], want + 0.0)
        np.testing.assert_array_equal(bq[b][rows].reshape(bt.nobs, H), dist[b] - np.asarray(bt.margin_cfs)[:, None])
    fd = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode="CFS", max_batch=B)
    A_f, _ = fd.get_con(x_, np.zeros((B, H * nj)), bt.xR1[:B], bt.obs[:B])
    assert np.abs(A_f - A).max() > 0                                # the mode really changes the rows
    an.close(); fd.close()


# ---- 3. every outer iteration --------------------------------------------------------------------------------------------
ONE_STEP_TOL = 1e-8          # as tests/test_gpu_chaos.py: |u_k(device) - qp(rows at u_{k-1}(device))|_inf / |u_k|_inf
KINK = 1e-9


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_every_iteration_uses_the_analytic_linearisation(gpu, O, c3, mode):
    check_every_iteration(gpu, O, c3, mode, "default")


def check_every_iteration(gpu, O, c3, mode, tier, idx=None, **kw):
    """the body of the test below; tier "w1": on the w1 tier, idx: other problems, kw: further handle options"""
    s, bt = c3
    idx = np.arange(64) if idx is None else np.asarray(idx)
    n, H, nj = idx.size, s.H, 5
    nn = H * nj
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    nz = bt.noise[idx] if (mode == "PSGCFS" and bt.noise is not None) else None
    slv = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=n, jacobian="analytic", **kw)
    if tier == "w1":                                                 # config 3's shape runs the half-CU tiers by default
        slv.debug_options(tier_w1=True)
    plain = slv.solve(bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx], noise=nz)
    slv.log_u(True)
    got = slv.solve(bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx], noise=nz)
    ulog = slv.read_u_log(n)
    for k in ("u", "x_", "status", "iter_O"):
        np.testing.assert_array_equal(getattr(plain, k), getattr(got, k), err_msg=k)
    dt = s.robot.delta_t
    jobs = []
    for a, b in enumerate(idx):
        n_it = int(got.iter_O[a]) - 1
        rows_used = 0
        for k in range(1, n_it + 1):
            u_prev = ulog[a, k - 2] if k >= 2 else np.zeros(nn)
            nz_row = None
            if mode == "PSGCFS":
                c = lambda j: (100000.0 if j < 0 else (bt.caug[b] if j == 0 else got.cost_all[a, j - 1]))   # noqa: E731
                if abs(c(k - 1) - c(k - 2)) < 1e-4:                  # stop_inner: no step
                    continue
                nz_row = bt.noise[b, rows_used] if bt.noise is not None and rows_used < bt.noise.shape[1] else None
                rows_used += 1
            jobs.append((a, int(b), k, u_prev, ulog[a, k - 1], nz_row))

    def step(b, k, u_prev, nz_row):
        x_ = bt.x_init[b] if k == 1 else O.rollout(H, nj, dt, bt.xR1[b], u_prev)
        A, rhs = slv.get_con(x_[None], u_prev[None], bt.xR1[b][None], bt.obs[b][None])
        A, rhs = A[0], rhs[0]
        if mode == "CFS":
            G, g0 = s.QQ, bt.ff[b]
            A = np.vstack([A, np.eye(nn), -np.eye(nn)])
            rhs = np.concatenate([rhs, s.MAX_input, s.MAX_input])
        else:
            z = np.zeros(nn) if nz_row is None else nz_row
            u_ = u_prev - s.alpha * ((s.QQ @ u_prev + bt.ff[b]) + 10.0 * z / (float(k) * float(k) + 1.0))
            G, g0 = np.eye(nn), -u_
        x, _, _, st, _ = O.qp_solve(G, g0, A, rhs)
        return x, st

    rng = np.random.default_rng(9)
    err, sens = [], []
    for a, b, k, u_prev, u_k, nz_row in jobs:
        want, st = step(b, k, u_prev, nz_row)
        w2, st2 = step(b, k, u_prev + (1e-12 * rng.standard_normal(nn) if k >= 2 else 0.0), nz_row) if k >= 2 else (want, st)
        sc = max(np.abs(u_k).max(), 1e-300)
        err.append(np.abs(u_k - want).max() / sc if st == 0 else np.inf)
        sens.append(np.abs(w2 - want).max() / sc if (st == 0 and st2 == 0) else np.inf)
    err, sens = np.array(err), np.array(sens)
    kink = ~(sens <= KINK)
    print(f"[{mode} {tier}] {len(jobs)} outer iterations of {n} analytic solves: {int(kink.sum())} kinked; un-kinked max {err[~kink].max():.1e}, "
          f"median {np.median(err[~kink]):.1e}")
    assert len(jobs) >= n
    assert (~kink).sum() >= 0.8 * len(jobs)
    assert err[~kink].max() <= ONE_STEP_TOL
    assert (err[kink] <= np.maximum(ONE_STEP_TOL, 1e3 * sens[kink])).mean() >= 0.98 if kink.any() else True
    slv.close()


# ---- 4. the default is untouched -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_fd_literal_is_bit_identical_to_the_default(gpu, c3, mode):
    s, bt = c3
    idx = np.arange(128)
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    nz = bt.noise[idx] if (mode == "PSGCFS" and bt.noise is not None) else None
    args = (bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx])
    ref = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=128).solve(*args, noise=nz)
    explicit = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=128, jacobian="fd_literal")
    sw = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=128, jacobian="analytic")
    an = sw.solve(*args, noise=nz)
    sw.set_jacobian("fd_literal")
    assert sw.jacobian == "fd_literal"
    for got in (explicit.solve(*args, noise=nz), sw.solve(*args, noise=nz)):
        for k in ("u", "x_", "status", "iter_O", "total_iter", "cost_all", "e_cost_all", "e_u_all"):
            np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert np.abs(an.x_ - ref.x_).max() > 0                         # (and the analytic solve is a different one)


def test_mesh_rows_do_not_depend_on_the_mode(gpu, O):
    M = gpu.mesh
    R, s, obs = gpu.main_FANUC_problem()
    tri = np.concatenate([M.cylinder_mesh((3.606, 8.413), 0.03, 0.0, 0.95, nseg=12, nring=6),
                          M.icosphere([3.606, 8.413, 1.0], 0.06, subdiv=2)]) + np.array([-0.25, 0.55, -0.3])
    g_obs = obs + [dict(mesh=gpu.Mesh(tri=tri), D=0.2, epsilon=0.25)]
    ref = gpu.CFS_FANUC(g_obs, s, R).optimizer()
    sw = gpu.CFS_FANUC(g_obs, s, R, jacobian="analytic")
    x_ = np.asarray(s.x_, float)[None]
    oa = gpu.obs_to_array(g_obs)[None]
    d_a, l_a, g_a = sw._batch.linearize(x_, oa)
    sw._batch.set_jacobian("fd_literal")
    d_f, l_f, g_f = sw._batch.linearize(x_, oa)
    np.testing.assert_array_equal(d_a, d_f)
    np.testing.assert_array_equal(g_a[:, -1], g_f[:, -1])           # the mesh obstacle's rows: cfs_mesh.hip's in both modes
    assert np.abs(g_a[:, 0] - g_f[:, 0]).max() > 0                  # the line obstacle's rows are the mode's
    got = sw.optimizer()                                            # switched back: the default solve, bit for bit
    np.testing.assert_array_equal(got.x_, ref.x_)
    assert got.status == ref.status and got.iter_O == ref.iter_O


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def test_main_fanuc_converges_in_analytic_mode(gpu):
    """SURVEY N8 puts the effect of num_jac's un-restored xp on the converged waypoints at ~6e-6 rad; the analytic derivative
    removes all of num_jac's O(eps) at once.  Measured: both converge in 10 iterations, 6.3e-6 rad apart."""
    R, s, obs = gpu.main_FANUC_problem()
    lit = gpu.CFS_FANUC(obs, s, R).optimizer()
    an = gpu.CFS_FANUC(obs, s, R, jacobian="analytic").optimizer()
    d = np.abs(an.x_ - lit.x_).max()
    print(f"main_FANUC CFS: analytic {gpu.STATUS[an.status]} in {an.iter_O - 1} iterations, literal in {lit.iter_O - 1}; "
          f"|x_ analytic - x_ literal|_inf = {d:.2e} rad")
    assert an.status == 0 and lit.status == 0
    assert d < 1e-4


E2E_STATUS_AGREE = 0.99      # measured 1.0000 in both solvers (1013 CFS / 969 PSGCFS non-chaotic problems)
E2E_LINF_MEDIAN = 1e-4       # measured median 1.1e-6 (CFS) / 2.6e-6 (PSGCFS) rad
E2E_LINF_P99 = 1e-2          # measured p99 6.2e-4 / 1.9e-3 rad, max 5.5e-3 / 6.0e-2 rad


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_config3_end_to_end(gpu, c3, c3_oracle, mode):
    """Config 3 without the problems helpers.chaotic_problems flags (on those a 1e-12 kick moves the answer by > 1e-6 rad, so
    an O(eps) change of the Jacobian can move it anywhere).  Status agreement with the literal mode and the l_inf waypoint
    difference on problems OK in both are asserted at the bounds above.  Measured (MI355X): status agreement 1.0000 in both
    solvers; |x_ analytic - x_ literal|_inf median 1.1e-6 / 2.6e-6 rad, p90 1.3e-5 / 2.8e-5, p99 6.2e-4 / 1.9e-3, max 5.5e-3 /
    6.0e-2 (CFS / PSGCFS), the same total outer iterations.  The Jacobians differ by up to 6.5e-5 (num_jac's O(eps) and its
    rounding), 1e7 times the 1e-12 kick that defines "chaotic", so a tail of problems still crosses a kink (a link switch, a
    clamp, an active-set change) on the way: the median and p99 are bounded, not the maximum."""
    s, bt = c3
    _, chaotic, _ = c3_oracle(mode)
    idx = np.nonzero(~chaotic)[0]
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    nz = bt.noise[idx] if (mode == "PSGCFS" and bt.noise is not None) else None
    args = (bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx])
    lit = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=idx.size).solve(*args, noise=nz)
    an = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=idx.size, jacobian="analytic").solve(*args, noise=nz)
    agree = (an.status == lit.status).mean()
    ok = (an.status <= 1) & (lit.status <= 1)
    dx = np.abs(an.x_ - lit.x_).max(axis=1)[ok]
    q = np.quantile(dx, [0.5, 0.9, 0.99, 1.0])
    print(f"[config3 {mode}] {idx.size} non-chaotic problems: status agreement {agree:.4f}; on {int(ok.sum())} OK in both, "
          f"|x_ analytic - x_ literal|_inf median {q[0]:.1e}, p90 {q[1]:.1e}, p99 {q[2]:.1e}, max {q[3]:.1e}; "
          f"iterations analytic {an.iter_O.sum()} vs literal {lit.iter_O.sum()}")
    assert agree >= E2E_STATUS_AGREE
    assert np.median(dx) < E2E_LINF_MEDIAN
    assert np.quantile(dx, 0.99) < E2E_LINF_P99


def test_2l_and_m16ib_end_to_end(gpu):
    """main_2L (point obstacle, zero-length in distLinSeg) and an M16iB three-obstacle problem: same status and iteration count
    as the literal mode, waypoints within 1e-3 rad.  Measured: 2L converges in 9 iterations in both modes, 3.4e-6 rad apart; the
    M16iB problem ends QP_INFEASIBLE at iteration 4 in both, its last iterates 2.1e-4 rad apart."""
    cases = []
    R, s, obs = gpu.main_2L_problem(lim=(1, 1))
    cases.append(("2L", R, s, obs))
    R, s, obs = gpu.main_FANUC_problem()
    th0 = np.array([0.5, 1.2, 0.1, 0.0, -1.2]); th1 = np.array([-0.5, 1.2, 0.1, 0.0, -1.2])
    r16 = gpu.robotproperty2("M16iB")
    s16 = gpu.build_sys_info(r16, 5, 20, th0, th1, gpu.line_reference(th0, th1, 20), Qp=np.diag([10.0, 10, 1, 1, 1]),
                             Qv=np.diag([10.0, 10, 1, 1, 1]), Rblk=np.eye(5) * 2, cR=50.0, lim=np.ones(5), max_input_blk=np.ones(5),
                             epsilon_O=0.1, MAX_O_ITER=20)
    ob3 = [gpu.cylinder((4300, 8500, 1), (4300, 8500, 1500), 0.2, 0.3), gpu.cylinder((2700, 8900, 1), (2700, 8900, 900), 0.2, 0.25),
           gpu.cylinder((3150, 7800, 1), (3150, 7800, 700), 0.2, 0.25)]
    cases.append(("M16iB x3", "M16iB", s16, ob3))
    for tag, R, s, obs in cases:
        lit = gpu.CFS_FANUC(obs, s, R).optimizer()
        an = gpu.CFS_FANUC(obs, s, R, jacobian="analytic").optimizer()
        d = np.abs(an.x_ - lit.x_).max()
        print(f"{tag}: literal {gpu.STATUS[lit.status]} / {lit.iter_O}, analytic {gpu.STATUS[an.status]} / {an.iter_O}, l_inf {d:.2e}")
        assert an.status == lit.status and an.iter_O == lit.iter_O
        assert d < 1e-3
